"""ctypes binding of libcaf.so (include/caf.h).

Follows the reference's own C-DLL idiom (cpuWola.py:38-70, cpuTone.py:28-47,
cython_ext/compareIntPreambles/compareIntPreambles.py:7-52): the shared library
sits next to the Python modules and is loaded with ``np.ctypeslib.load_library``;
every entry point returns an int32 status (0 = success) and writes into
caller-allocated buffers.

There is NO CPU fallback: if the library is missing or a call fails, the host
raises.  The oracle under ``oracle/`` is test infrastructure and is never
imported from here.
"""

import ctypes as ct
import os

import numpy as np

_HERE = os.path.dirname(os.path.realpath(__file__))

CAF_OK = 0
CAF_ERR_INVALID = 1
CAF_ERR_HIP = 2
CAF_ERR_ROCFFT = 3
CAF_ERR_NOMEM = 4
CAF_ERR_NODEVICE = 5

CAF_FREQ_BINS = 0
CAF_FREQ_NORM = 1
CAF_ENGINE_AUTO = 0
CAF_ENGINE_ROCFFT = 1
CAF_ENGINE_FUSED = 2
CAF_ENGINE_PERSISTENT = 3
CAF_ENGINE_DIRECT = 4
ENGINE_IDS = {
    "auto": CAF_ENGINE_AUTO,
    "rocfft": CAF_ENGINE_ROCFFT,
    "fused": CAF_ENGINE_FUSED,
    "persistent": CAF_ENGINE_PERSISTENT,
    "direct": CAF_ENGINE_DIRECT,
}
ENGINE_NAMES = {v: k for k, v in ENGINE_IDS.items() if k != "auto"}
CAF_NUM_STAGES = 7
STAGE_NAMES = (
    "energy_prefix",
    "gather_blocks",
    "fft_forward",
    "spectral_conj_multiply",
    "fft_inverse(rocFFT)",
    "magsq_norm_argmax",
    "peak_reduce",
)


class CafPlanDesc(ct.Structure):
    _fields_ = [
        ("num_templates", ct.c_int32),
        ("template_len", ct.c_int32),
        ("h_templates", ct.c_void_p),
        ("auto_conj", ct.c_int32),
        ("num_groups", ct.c_int32),
        ("h_group_start", ct.c_void_p),
        ("h_group_len", ct.c_void_p),
        ("freq_mode", ct.c_int32),
        ("num_freqs", ct.c_int32),
        ("h_bins", ct.c_void_p),
        ("grid", ct.c_int32),
        ("h_freqs_norm", ct.c_void_p),
        ("max_rx_len", ct.c_int64),
        ("log2_block", ct.c_int32),
        ("blocks_per_batch", ct.c_int32),
        ("engine", ct.c_int32),
        ("reserved", ct.c_int32),
    ]


class CafOutputs(ct.Structure):
    _fields_ = [
        ("d_surface", ct.c_void_p),
        ("d_row_max", ct.c_void_p),
        ("d_row_arg", ct.c_void_p),
        ("d_peak_val", ct.c_void_p),
        ("d_peak_delay", ct.c_void_p),
        ("d_peak_freq", ct.c_void_p),
        ("d_cqf", ct.c_void_p),
    ]


class CafOutputs2(ct.Structure):
    _fields_ = [("base", CafOutputs), ("d_surface_t", ct.c_void_p), ("reserved", ct.c_void_p * 3)]


class CafZoomOutputs(ct.Structure):
    _fields_ = [
        ("d_count", ct.c_void_p),
        ("d_delay", ct.c_void_p),
        ("d_coarse_freq_index", ct.c_void_p),
        ("d_coarse_qf2", ct.c_void_p),
        ("d_fine_index", ct.c_void_p),
        ("d_fine_freq", ct.c_void_p),
        ("d_fine_qf2", ct.c_void_p),
        ("d_planes", ct.c_void_p),
    ]


class CafDemodDesc(ct.Structure):
    _fields_ = [
        ("d_x", ct.c_void_p),
        ("rows", ct.c_int64),
        ("xlength", ct.c_int64),
        ("osr", ct.c_int32),
        ("m", ct.c_int32),
        ("d_m", ct.c_void_p),
        ("d_lengths", ct.c_void_p),
        ("d_abs", ct.c_void_p),
        ("lock", ct.c_int32),
        ("map", ct.c_int32),
        ("d_syms", ct.c_void_p),
        ("d_eo_index", ct.c_void_p),
        ("d_eo_metric", ct.c_void_p),
        ("d_angle", ct.c_void_p),
        ("d_svd", ct.c_void_p),
        ("d_moments", ct.c_void_p),
        ("d_reimc", ct.c_void_p),
        ("d_xeo", ct.c_void_p),
        ("xeo_pitch", ct.c_int64),
        ("eye_only", ct.c_int32),
        ("num_preambles", ct.c_int32),
        ("d_preambles", ct.c_void_p),
        ("d_preamble_lengths", ct.c_void_p),
        ("preamble_total", ct.c_int32),
        ("max_preamble_length", ct.c_int32),
        ("search_start", ct.c_int32),
        ("search_end", ct.c_int32),
        ("d_best", ct.c_void_p),
        ("d_payload", ct.c_void_p),
        ("d_count", ct.c_void_p),
        ("out_length", ct.c_int64),
        ("scaling", ct.c_float),
        ("reserved", ct.c_int32),
    ]


class CafLocateDesc(ct.Structure):
    _fields_ = [
        ("source", ct.c_int32),
        ("mode", ct.c_int32),
        ("cost_f32", ct.c_int32),
        ("reserved", ct.c_int32),
        ("n", ct.c_int64),
        ("d_points", ct.c_void_p),
        ("ni", ct.c_int32),
        ("nj", ct.c_int32),
        ("d_a", ct.c_void_p),
        ("d_z", ct.c_void_p),
        ("d_c", ct.c_void_p),
        ("d_s", ct.c_void_p),
        ("z", ct.c_double),
    ]


class CafDpdMap(ct.Structure):
    _fields_ = [
        ("d_surface", ct.c_void_p),
        ("nd", ct.c_int32),
        ("nf", ct.c_int32),
        ("stride_d", ct.c_int64),
        ("stride_f", ct.c_int64),
        ("r0", ct.c_double),
        ("inv_dr", ct.c_double),
        ("d0", ct.c_double),
        ("inv_dd", ct.c_double),
        ("w", ct.c_double),
        ("fill", ct.c_double),
    ]


class CafDpdDesc(ct.Structure):
    _fields_ = [
        ("grid", CafLocateDesc),
        ("d_records", ct.c_void_p),
        ("K", ct.c_int64),
        ("d_set_starts", ct.c_void_p),
        ("B", ct.c_int32),
        ("reserved", ct.c_int32),
        ("h_maps", ct.c_void_p),
        ("d_score", ct.c_void_p),
        ("d_hits", ct.c_void_p),
        ("d_max_val", ct.c_void_p),
        ("d_max_idx", ct.c_void_p),
        ("stream", ct.c_void_p),
    ]


class CafCfarMap(ct.Structure):
    _fields_ = [
        ("d_surface", ct.c_void_p),
        ("nd", ct.c_int32),
        ("nf", ct.c_int32),
        ("stride_d", ct.c_int64),
        ("stride_f", ct.c_int64),
        ("alpha", ct.c_double),
        ("floor", ct.c_double),
        ("d_noise", ct.c_void_p),
    ]


class CafCfarDet(ct.Structure):
    _fields_ = [
        ("i", ct.c_int32),
        ("j", ct.c_int32),
        ("value", ct.c_float),
        ("noise", ct.c_float),
        ("ratio", ct.c_float),
        ("di", ct.c_float),
        ("dj", ct.c_float),
        ("cells", ct.c_int32),
    ]


class CafCfarDesc(ct.Structure):
    _fields_ = [
        ("h_maps", ct.c_void_p),
        ("B", ct.c_int32),
        ("gd", ct.c_int32),
        ("gf", ct.c_int32),
        ("td", ct.c_int32),
        ("tf", ct.c_int32),
        ("md", ct.c_int32),
        ("mf", ct.c_int32),
        ("mode", ct.c_int32),
        ("split_axis", ct.c_int32),
        ("wrap_f", ct.c_int32),
        ("min_cells", ct.c_int32),
        ("d_det", ct.c_void_p),
        ("cap", ct.c_int64),
        ("d_count", ct.c_void_p),
        ("stream", ct.c_void_p),
    ]


class CafLopDesc(ct.Structure):
    _fields_ = [
        ("kind", ct.c_int32),
        ("spacing", ct.c_int32),
        ("P", ct.c_int32),
        ("reserved", ct.c_int32),
        ("omega", ct.c_double),
        ("lambda_", ct.c_double),
        ("d_p", ct.c_void_p),
    ]


class CafViterbiDesc(ct.Structure):
    _fields_ = [
        ("num_states", ct.c_int32),
        ("num_trans", ct.c_int32),
        ("up", ct.c_int32),
        ("pulselen", ct.c_int32),
        ("pathlen", ct.c_int32),
        ("num_burst_syms", ct.c_int32),
        ("num_guard_syms", ct.c_int32),
        ("y_c128", ct.c_int32),
        ("h_alphabet", ct.c_void_p),
        ("h_pretransitions", ct.c_void_p),
        ("h_allowed", ct.c_void_p),
        ("num_allowed", ct.c_int32),
        ("reserved", ct.c_int32),
        ("d_table", ct.c_void_p),
        ("d_y", ct.c_void_p),
        ("rows", ct.c_int64),
        ("ylength", ct.c_int64),
        ("d_states", ct.c_void_p),
        ("d_metrics", ct.c_void_p),
        ("d_best", ct.c_void_p),
        ("d_best_path", ct.c_void_p),
    ]


class CafTrajTable(ct.Structure):
    _fields_ = [
        ("count", ct.c_int32),
        ("reserved", ct.c_int32),
        ("h_kind", ct.c_void_p),
        ("h_x0v", ct.c_void_p),
        ("h_knot_off", ct.c_void_p),
        ("d_tp", ct.c_void_p),
        ("d_xp", ct.c_void_p),
    ]


class CafBurstTable(ct.Structure):
    _fields_ = [
        ("count", ct.c_int32),
        ("reserved", ct.c_int32),
        ("h_burst_off", ct.c_void_p),
        ("h_burst", ct.c_void_p),
        ("h_phase_off", ct.c_void_p),
        ("d_phase", ct.c_void_p),
    ]


class CafScfDesc(ct.Structure):
    _fields_ = [
        ("d_x", ct.c_void_p),
        ("rows", ct.c_int64),
        ("pitch", ct.c_int64),
        ("n", ct.c_int64),
        ("num_channels", ct.c_int32),
        ("hop", ct.c_int32),
        ("num_hops", ct.c_int32),
        ("conjugate", ct.c_int32),
        ("coherence", ct.c_int32),
        ("reserved", ct.c_int32),
        ("d_window", ct.c_void_p),
        ("d_smooth", ct.c_void_p),
        ("stream", ct.c_void_p),
    ]


class CafScfOutputs(ct.Structure):
    _fields_ = [
        ("d_scf", ct.c_void_p),
        ("d_alpha_val", ct.c_void_p),
        ("d_alpha_arg", ct.c_void_p),
        ("d_psd", ct.c_void_p),
    ]


class CafResampleDesc(ct.Structure):
    _fields_ = [
        ("d_x", ct.c_void_p),
        ("rows", ct.c_int64),
        ("pitch", ct.c_int64),
        ("h_lengths", ct.c_void_p),
        ("h_nu", ct.c_void_p),
        ("h_t0", ct.c_void_p),
        ("h_step", ct.c_void_p),
        ("h_width", ct.c_void_p),
        ("h_counts", ct.c_void_p),
        ("d_table", ct.c_void_p),
        ("half_width", ct.c_int32),
        ("phases", ct.c_int32),
        ("d_y", ct.c_void_p),
        ("out_pitch", ct.c_int64),
        ("stream", ct.c_void_p),
    ]


CAF_TRAJ_STATIONARY = 0
CAF_TRAJ_CONSTANT_VELOCITY = 1
CAF_TRAJ_INTERPOLATED = 2

CAF_LOCATE_POINTS = 0
CAF_LOCATE_MESH = 1
CAF_LOCATE_MESH_XY = 2
CAF_LOCATE_TD = 1
CAF_LOCATE_FD = 2
CAF_LOCATE_TDFD = 3
CAF_CFAR_CA = 0
CAF_CFAR_GO = 1
CAF_CFAR_SO = 2
CAF_CRB_RANGE, CAF_CRB_RANGE_SUM, CAF_CRB_RANGE_DIFF, CAF_CRB_RATE_DIFF, CAF_CRB_AOA3D = 1, 2, 3, 4, 5
CAF_CRB_FREE, CAF_CRB_FIXED, CAF_CRB_RADIAL, CAF_CRB_WGS84 = 0, 1, 2, 3
CAF_LOP_HYPERBOLOID, CAF_LOP_SPHERE = 0, 1
CAF_LOP_LIST, CAF_LOP_LINSPACE, CAF_LOP_CHEBYSHEV = 0, 1, 2
CAF_LOP_FOUND, CAF_LOP_NO_CURVE = 0, 1

CAF_DEMOD_LOCK_EIG = 0
CAF_DEMOD_LOCK_POWERSUM = 1
CAF_DEMOD_LOCK_NONE = 2
CAF_DEMOD_MAP_CLASS = 0
CAF_DEMOD_MAP_GENERIC = 1
CAF_DEMOD_MAP_SIGNBITS = 2
CAF_DEMOD_MAP_GRAYBATCH = 3

_P = ct.c_void_p
_I32 = ct.c_int32
_I64 = ct.c_int64

# name -> argtypes; restype is always int32 (the reference DLL convention)
_SIGNATURES = {
    "caf_last_error": [ct.c_char_p, _I32],
    "caf_abi_version": [],
    "caf_xcorr_perdelay_one_kernel": [_I32],
    "caf_perdelay_jit_describe": [_I32, ct.c_char_p, ct.c_char_p, ct.c_char_p, _I32],
    "caf_device_count": [ct.POINTER(_I32)],
    "caf_set_device": [_I32],
    "caf_device_info": [_I32, ct.c_char_p, _I32, ct.POINTER(_I64), ct.POINTER(_I32)],
    "caf_malloc": [ct.POINTER(_P), _I64],
    "caf_free": [_P],
    "caf_pool_trim": [],
    "caf_pool_stats": [ct.POINTER(_I64), ct.POINTER(_I64), ct.POINTER(_I64), ct.POINTER(_I64)],
    "caf_memset": [_P, _I32, _I64, _P],
    "caf_h2d": [_P, _P, _I64, _P],
    "caf_d2h": [_P, _P, _I64, _P],
    "caf_d2d": [_P, _P, _I64, _P],
    "caf_d2h_transposed": [_P, _I32, _P, _I64, _I64, _I64, _I64, _P],
    "caf_d2h_f64": [_P, _P, _I64, _P],
    "caf_stream_sync": [_P],
    "caf_stream_create": [ct.POINTER(_P)],
    "caf_stream_destroy": [_P],
    "caf_plan_create": [ct.POINTER(_P), ct.POINTER(CafPlanDesc)],
    "caf_plan_destroy": [_P],
    "caf_plan_info": [_P, ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I64)],
    "caf_plan_engine": [_P, ct.POINTER(_I32)],
    "caf_plan_execute": [_P, _P, _I64, _I64, _I64, ct.POINTER(CafOutputs), _P],
    "caf_plan_execute2": [_P, _P, _I64, _I64, _I64, ct.POINTER(CafOutputs2), _P],
    "caf_plan_watchdog": [_P, ct.POINTER(_I32)],
    "caf_plan_profile": [_P, _I32],
    "caf_plan_profile_get": [_P, ct.POINTER(ct.c_double), ct.POINTER(_I64)],
    "caf_plan_execute_host": [_P, _P, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P],
    "caf_xcorr_perdelay": [_P, _I32, _P, _I64, _I64, _I64, _I64, _I32, _P, _P, _P, _P, _I64, _P],
    "caf_fft_rows": [_P, _P, _I64, _I64, _I32, _P],
    "caf_sliding_multiply_normalised": [_P, _I32, _P, _I64, _I64, _I64, ct.c_double, _P, _P],
    "caf_multi_template_sliding_dot": [_P, _P, _I32, _I32, _P, _I64, _I64, _I64, _P, _P, _P],
    "caf_multiply_slices_indexed_rows": [_P, _I64, _P, _I32, _I32, _P, _P, _P, _I32, _I64, _P, _P],
    "caf_complex_magnsq": [_P, _I64, _I32, _P, _I32, _P],
    "caf_argmax_abs_rows": [_P, _I64, _I64, _P, _P, _I32, _P],
    "caf_moving_average": [_P, _I64, _I64, _I32, _I32, _P, _P],
    "caf_complex_moving_sum": [_P, _I64, _I32, _P, _P],
    "caf_copy_slices_to_matrix": [_P, _I64, _P, _I32, _I64, _I64, _I32, _I64, _P, _P],
    "caf_copy_groups": [_P, _P, _P, _P, _P, _I32, _P],
    "caf_find_local_maxima": [_P, _I64, ct.c_float, _I32, _P, _P, _P],
    "caf_gather_b32": [_P, _I64, _P, _I64, _P, _P],
    "caf_gather_f32_f64": [_P, _I64, _P, _I64, _P, _P],
    "caf_fir_lfilter": [_P, _I64, _P, _I32, _P, _I32, _I32, _I32, _P, _I64, _P],
    "caf_wola": [_P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _I64, _P],
    "caf_abs_ampsq": [_P, _I64, _I32, _P, _P, _P],
    "caf_medfilt": [_P, _I64, _I32, _I64, _P, _P],
    "caf_threshold_edges": [_P, _I64, ct.c_float, _I32, _I32, _P, _P, _P],
    "caf_gather_edges": [_P, _I64, _I32, _P, _I32, _I32, _P, _I64, ct.POINTER(_I64), _P],
    "caf_threshold_indices": [_P, _I64, _I32, ct.c_double, _P, _I64, _P, _I64, ct.POINTER(_I64), _P],
    "caf_histogram": [_P, _I64, _I32, _P, _I64, _P, _P],
    "caf_column_means": [_P, _I64, _I64, _I32, _I32, _P, _P],
    "caf_upfirdn": [_P, _I64, _I64, _P, _I32, _I32, _I32, _P, _P, _I64, _P],
    "caf_czt_run_many": [_P, _I64, _I32, _I32, _I32, _P, _P, _P, _P, _P],
    "caf_argmax3d_u32": [_P, _I64, _I32, _I32, _I32, _P, _P, _P],
    "caf_iq16_to_c64": [_P, _I64, ct.c_float, _P, _P],
    "caf_iq16_fir_decimate": [_P, _I64, ct.c_float, _P, _I32, _P, _I32, _I32, _I32, _P, _I64, _P],
    "caf_colmax_abs": [_P, _I32, _I64, _P, _P, _I32, _P],
    "caf_colmax_sqrt": [_P, _I32, _I64, _P, _P, _P],
    "caf_dot_tones": [_P, _I64, ct.c_double, ct.c_double, _I32, _P, _P],
    "caf_mul_conj": [_P, _P, _I64, _P, _P],
    "caf_steer_dot": [_P, _P, _I64, _I64, ct.c_double, _P, _P],
    "caf_sum_planes_qf2": [_P, _I32, _I64, _I32, _P, _I32, _P, ct.c_double, _P, _P],
    "caf_sum_groups_qf2": [_P, _I32, _I64, _I32, _P, _P, ct.c_double, _P, _P],
    "caf_comm_unique_id": [_P],
    "caf_comm_create": [ct.POINTER(_P), _I32, _I32, _P],
    "caf_comm_destroy": [_P],
    "caf_peak_table_allgather": [_P, _P, _I32, _P, _P],
    "caf_zoom_num_bins": [ct.c_double, ct.c_double, ct.POINTER(_I32)],
    "caf_zoom_czt": [_P, _I32, _P, _I64, _P, _P, _I64, _I64, _I32, ct.c_float, ct.c_double, ct.c_double,
                     ct.POINTER(CafZoomOutputs), _P],
    "caf_psk_demod_rows": [ct.POINTER(CafDemodDesc), _P],
    "caf_eye_opening_batch": [_P, _P, _I64, _I64, _I32, _P, _I64, _P, _P, _P],
    "caf_compare_int_preambles": [_P, _I64, _I64, _I32, _I32, _P, _I32, _P, _I32, _I32, _I32, _P, _P, _P],
    "caf_cut_rotate_gray": [_P, _I64, _P, _I64, _P, _I32, _P, _I32, _I64, _P, _P, _P, _P],
    "caf_amble_search_bits": [_P, _I64, _I64, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P],
    "caf_cp2fsk_tone_metric": [_P, _I64, _I64, _I32, ct.c_double, _I64, _I64, _I64, _P, _P, _P, _P, _P],
    "caf_cp2fsk_comb_costs": [_P, _I64, _I64, _I32, _I32, _P, _I32, _I64, _I64, _P, _P],
    "caf_cp2fsk_bursty_demod": [_P, _I64, _I64, _I32, ct.c_double, _I32, _P, _I32, _I64, _I64, _P, _P, _P, _P],
    "caf_locate_grid": [ct.POINTER(CafLocateDesc), _P, _I64, _P, _I32, _P, _P, _P, _P],
    "caf_locate_geometry": [ct.POINTER(_I32), ct.POINTER(_I32)],
    "caf_locate_rtt": [ct.POINTER(CafLocateDesc), _P, _I64, _P, _I32, _I32, _P, _P, _P, _P],
    "caf_locate_rtt_geometry": [ct.POINTER(_I32), ct.POINTER(_I32)],
    "caf_crb_map": [ct.POINTER(CafLocateDesc), _P, _I64, _P, _I32, _I32, ct.POINTER(ct.c_double), _P, _P, _P, _P, _P, _P, _P, _P],
    "caf_crb_map_geometry": [ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(ct.c_double)],
    "caf_dpd_grid": [ct.POINTER(CafDpdDesc)],
    "caf_dpd_geometry": [ct.POINTER(_I32), ct.POINTER(_I32)],
    "caf_cfar_surface": [ct.POINTER(CafCfarDesc)],
    "caf_cfar_geometry": [_I32, _I32, ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I64)],
    "caf_lop_points": [ct.POINTER(CafLopDesc), _P, _I64, _P, _P, _P, _P, _P, _P, _P],
    "caf_lop_range": [ct.POINTER(CafLopDesc), _P, _I64, _P, _P, _P],
    "caf_lop_geometry": [ct.POINTER(_I32)] * 4,
    "caf_viterbi_table": [_P, _P, _I32, _I32, _I32, _I32, _P, _P],
    "caf_viterbi_demod": [ct.POINTER(CafViterbiDesc), _P],
    "caf_viterbi_geometry": [ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32)],
    "caf_propagate": [_P, _I32, _I64, _P, _I32, ct.c_double, _P, _P, _P],
    "caf_propagate_exact": [_P, _P, _I32, _I32, ct.c_double, ct.c_double, _P, _P],
    "caf_propagate_geometry": [ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32)],
    "caf_gen_tones": [ct.c_double, ct.c_double, _I32, _I64, _I32, _P, _P],
    "caf_add_tone_phase": [_P, _I64, ct.c_double, ct.c_double, ct.c_double, _P],
    "caf_freq_shift": [_P, _I64, _I64, ct.c_double, _P, _P],
    "caf_music_geometry": [ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32)],
    "caf_music_cov": [_P, _I32, _I64, _P, _I32, _I32, _I32, _I64, _P, _I32, _I32, _P, _P],
    "caf_music_eig": [_P, _I32, _I32, _P, _P, _P, _P, _P],
    "caf_music_spectrum": [_P, _P, _I32, _I32, _P, _I32, _P, _I32, _I32, _P, _P, _P, _P],
    "caf_music_xcorr_front": [_P, _I64, _P, _I64, _P, _I32, _P, _I32, _P, _P],
    "caf_scene_geometry": [ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I64), ct.POINTER(_I32), ct.POINTER(_I32)],
    "caf_traj_tau": [ct.POINTER(CafTrajTable), ct.POINTER(CafTrajTable), _P, _I64, _I32, _I32, _P, _P],
    "caf_lerp_propagate": [ct.POINTER(CafBurstTable), _P, _P, _I64, _I64, _I32, _P, _P],
    "caf_scene_propagate": [ct.POINTER(CafTrajTable), ct.POINTER(CafTrajTable), ct.POINTER(CafBurstTable), ct.c_double, ct.c_double,
                            _I64, _I32, _P, _P],
    "caf_cancel_geometry": [ct.POINTER(_I32)] * 7,
    "caf_cancel_search": [_P, _I32, _I32, _P, _I64, _P, ct.c_double, ct.c_double, _I32, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                          _P, _P],
    "caf_cancel_estimate": [_P, _I32, _I32, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "caf_cancel_subtract": [_P, _I32, _I32, _P, _I64, _P, _P, _P, _P, _P, _P],
    "caf_mp_geometry": [_I64, _I32, _I64] + [ct.POINTER(_I32)] * 4 + [ct.POINTER(_I64)] * 4,
    "caf_mp_raw": [_P, _I64, _I32, _I32, _I32, _P, _P],
    "caf_mp_chains": [_P, _I64, _I32, _I32, _I32, _P, _I32, ct.c_float, _I64, _P, ct.POINTER(_I64), _P],
    "caf_mp_profile": [_P, _I64, _I32, _I32, _I32, _P, _P, _P],
    "caf_cm_geometry": [_I64] + [ct.POINTER(_I32)] * 3 + [ct.POINTER(_I64)],
    "caf_cm_lines": [_P, _I64, _I64, _P, _I64, ct.POINTER(_I32), _I32, ct.POINTER(_I32), ct.POINTER(_I32), _P, _P, _P, _P, _P],
    "caf_scf_fam": [ct.POINTER(CafScfDesc), ct.POINTER(CafScfOutputs)],
    "caf_scf_geometry": [_I32, _I32, _I32, ct.POINTER(_I32), ct.POINTER(_I64), ct.POINTER(_I64), ct.POINTER(_I32), ct.POINTER(_I64),
                         ct.POINTER(_I64)],
    "caf_resample_rows": [ct.POINTER(CafResampleDesc)],
    "caf_resample_geometry": [_I32, _I32, ct.c_double, ct.c_double, ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I64)],
    "caf_cluster_geometry": [_I64, _I32, _I32] + [ct.POINTER(_I32)] * 3 + [ct.POINTER(_I64)] * 3,
    "caf_kmeans_seed": [_P, _I64, _I64, _I32, _P, _P, ct.POINTER(_I32), ct.POINTER(_I32), _I64, _I32, _P, _P, _P, _P],
    "caf_kmeans_lloyd": [_P, _I64, _I64, _I32, _P, _P, ct.POINTER(_I32), ct.POINTER(_I32), _I64, _I32, _I32, _P, _P, _P, _P, _P, _P, _P],
    "caf_cluster_scores": [_P, _I64, _I64, _I32, _P, ct.POINTER(_I32), ct.POINTER(_I32), _I64, _I32, _P, ct.POINTER(_I32), _I64, ct.c_uint32, _P, _P, _P, _P, _P],
    "caf_tone_spectrum": [_P, _P, _P, _I64, _P, _I64, ct.c_double, _I64, _P, _P],
    "caf_tone_spectrum_one": [ct.c_double, ct.c_double, ct.c_double, _P, _I64, ct.c_double, _I64, _P, _P],
    "caf_dft_rows": [_P, _I32, _I64, _I64, _P, _I64, ct.c_double, _P, _P],
    "caf_dft_geometry": [ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I64), ct.POINTER(_I32)],
    "caf_integer_multiple_fft": [_P, _I64, _I64, _I32, _I32, _P, _P],
    "caf_burst_fft": [_P, _I64, _I64, _I64, _P, _P],
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def _share_rocm_runtime_with_torch():
    """One HIP runtime per process.

    PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so / librocfft.so under torch/lib and ask
    for them by file name ("libamdhip64.so", RPATH $ORIGIN), while libcaf.so asks for the soname ("libamdhip64.so.7").
    If torch is imported AFTER libcaf.so has pulled in the system ROCm, the dynamic linker does not recognise the two
    as the same library and the process ends up with two HIP + two HSA runtimes: torch then reports "no ROCm-capable
    device" and the interpreter aborts in free() while both tear down at exit.  With the bundled copies loaded first,
    libcaf's soname requests and torch's file-name requests resolve to the same objects in either import order.
    Nothing is imported from torch here; CAF_SYSTEM_ROCM=1 keeps the system runtime (a process that never loads torch).
    """
    import sys

    if os.environ.get("CAF_SYSTEM_ROCM") == "1" or "torch" in sys.modules:
        return  # torch already loaded: its runtime is in the process and libcaf's sonames bind to it
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so", "librocfft.so", "librccl.so"):  # rccl: caf_comm_* dlopens its soname
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            ct.CDLL(path)  # RTLD_LOCAL: global scope would interpose the amd::smi statics of libamd_smi


MIN_HW_QUEUES = 16


def _enough_hardware_queues():
    """Streams beyond GPU_MAX_HW_QUEUES (HIP's default: 4) share a hardware queue, and work on a stream then waits behind
    whatever an unrelated stream on the same queue has queued: a plan's auxiliary stream behind the caller's ingest stream, the
    null stream's downloads behind an auxiliary stream that waits for the caller's.
    The library keeps up to 16 auxiliary streams beside the callers' own and promises calls that are asynchronous on the
    caller's stream, so it asks for at least MIN_HW_QUEUES queues.  The runtime reads the variable when it
    initialises: this has to run before the first HIP call of the process (a client that has initialised HIP already keeps what
    it had: INTEGRATION.md), and a larger value that is already set is kept.  A smaller one is raised, also one set on purpose:
    with fewer queues than streams the header's promise does not hold, and child processes inherit the larger value."""
    try:
        cur = int(os.environ.get("GPU_MAX_HW_QUEUES", "0"))
    except ValueError:
        cur = 0
    if cur < MIN_HW_QUEUES:
        os.environ["GPU_MAX_HW_QUEUES"] = str(MIN_HW_QUEUES)


def load():
    """Load libcaf.so (once).  Raises OSError with build instructions if absent."""
    global _lib
    if _lib is not None:
        return _lib
    _enough_hardware_queues()
    _share_rocm_runtime_with_torch()
    try:
        # CAF_LIBRARY=<name>: a development switch for A/B runs of two builds on one box (e.g. libcaf_r02, kept beside
        # libcaf.so); the product always loads libcaf.so
        lib = np.ctypeslib.load_library(os.environ.get("CAF_LIBRARY", "libcaf"), _HERE)
    except OSError as e:
        raise OSError(
            "pydsproutines_amd: libcaf.so (the HIP extension) is missing or cannot be loaded from %s "
            "(%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C pydsproutines_amd/csrc`. There is no CPU fallback." % (_HERE, e)
        ) from e
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = _I32
        fn.argtypes = argtypes
    _lib = lib
    return lib


def last_error():
    buf = ct.create_string_buffer(1024)
    load().caf_last_error(buf, 1024)
    return buf.value.decode("utf-8", "replace")


def check(rc, what=""):
    """Map a libcaf status to the reference's exception types
    (ValueError shape/range, MemoryError resource, RuntimeError 'DLL returned an error')."""
    if rc == CAF_OK:
        return
    msg = "%s: %s" % (what or "libcaf", last_error())
    if rc == CAF_ERR_INVALID:
        raise ValueError(msg)
    if rc == CAF_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError("DLL returned an error. " + msg)


# ------------------------------------------------------------------------------------------------------------------ the binding
# How every module above libcaf.so calls it: coercion, status check, out-parameters and the lifetime of what a
# wrapper uploads for one call are written here once.


def ptr(a):
    """c_void_p of a device array (anything with .ptr); None stays None"""
    return None if a is None else ct.c_void_p(a.ptr)


def stream_arg(stream):
    """a caller's stream as ctypes takes it: None (the null stream), a c_void_p, or the handle as an int"""
    if stream is None or isinstance(stream, ct.c_void_p):
        return stream
    return ct.c_void_p(int(stream))


_POINTERS = {}  # name -> the positions of its pointer parameters: call() looks at these alone (most arguments are numbers)
_ADDRESSES = frozenset((type(None), int, ct.c_void_p))  # what a pointer parameter takes as it is
_NO_STREAM = object()


def call(name, *args, stream=_NO_STREAM):
    """libcaf's `name` on `args`: device arrays go as their pointers, structures by reference, `stream=` (for the functions that
    take one) last; a status other than CAF_OK raises under the function's name."""
    args = list(args)
    if stream is not _NO_STREAM:
        args.append(stream if stream is None else stream_arg(stream))
    try:
        pointers = _POINTERS[name]
    except KeyError:
        pointers = _POINTERS[name] = [i for i, t in enumerate(_SIGNATURES[name]) if t is _P or issubclass(t, ct._Pointer)]
    for i in pointers:
        a = args[i]
        if type(a) not in _ADDRESSES:
            try:
                args[i] = _P(a.ptr)
            except AttributeError:  # (ctypes arrays, pointers and references go as they are)
                if isinstance(a, ct.Structure):
                    args[i] = ct.byref(a)
    rc = getattr(load(), name)(*args)
    if rc:
        check(rc, name)


def malloc(nbytes):
    """the address of a block from the library's pool.  Every wrapper allocates its outputs, so this one call skips call()'s look
    at the arguments (profiles/r24/bench_ab.txt)"""
    p = _P()
    rc = load().caf_malloc(ct.byref(p), nbytes)
    if rc:
        check(rc, "caf_malloc")
    return p.value or 0


def query(name, *ins):
    """the values of `name`'s out-parameters as a tuple: one scalar per POINTER(scalar) entry of its signature after `ins`"""
    outs = [t._type_() for t in _SIGNATURES[name][len(ins):]]
    call(name, *ins, *[ct.byref(o) for o in outs])
    return tuple(o.value for o in outs)


def drain(stream):
    """wait until `stream` (None: the null stream) has run dry"""
    call("caf_stream_sync", stream=stream)


def download(arr, stream, null_too=False):
    """the host copy of a result queued on `stream`: the stream is drained first (the download runs on the null stream, which a
    caller's stream is not ordered with); the null stream itself only where the site says so"""
    if null_too or stream is not None:
        drain(stream)
    return arr.get()


IF_UPLOADED, CALLER, ALWAYS = "caller's stream, if something was uploaded", "caller's stream", "always, null stream included"


class held:
    """What a wrapper uploads for one call, kept until the stream is done with it.  A block that goes back to the pool under a
    kernel queued on a caller's stream is handed to the pool's next user while that kernel still reads it (the pool looks after
    the null stream alone: caf_pool.hip), so on the way out the stream is drained by the site's rule (IF_UPLOADED, CALLER or
    ALWAYS) and only then are the uploads let go.  On the way out through an exception the
    rule does not count: whatever was uploaded is drained, on the null stream too."""

    def __init__(self, stream, rule):
        if not any(rule is r for r in (IF_UPLOADED, CALLER, ALWAYS)):
            raise ValueError("held: the rule is one of _lib.IF_UPLOADED, _lib.CALLER and _lib.ALWAYS, found %r" % (rule,))
        self.stream, self.rule, self.uploads = stream, rule, []

    def put(self, x, dtype=None):
        """x if it is on the device already, else its upload"""
        from .devarray import DeviceArray, asarray  # (devarray imports this module)

        if isinstance(x, DeviceArray):
            return x
        self.uploads.append(asarray(x, dtype=dtype))
        return self.uploads[-1]

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is not None:
                if self.uploads:
                    drain(self.stream)
            elif self.rule is ALWAYS or (self.rule is CALLER or self.uploads) and self.stream is not None:
                drain(self.stream)
        finally:
            del self.uploads[:]
        return False


def device_count():
    """0 when the library cannot say (no raise: require_device words the refusal), and on every wrapper's path through
    require_device, so it keeps its direct call"""
    n = _I32(0)
    rc = load().caf_device_count(ct.byref(n))
    return n.value if rc == CAF_OK else 0


def require_device():
    """Fail loudly when no GPU is usable (no silent CPU path)."""
    if device_count() < 1:
        raise RuntimeError("pydsproutines_amd: no MI355X/HIP device visible: " + last_error())
