/*
 * libcaf -- C-ABI of the MI355X (gfx950) cross-ambiguity-function / matched-filter engine.
 *
 * This header is the drop-in boundary.  It follows the reference's own C-DLL idiom
 * (icyveins7/pydsproutines cpuWola.py:38-70 + cpuWolaDll.c:107, cpuTone.py:28-47 +
 * cpuToneDll.c:33, cython_ext/compareIntPreambles/compareIntPreambles.py:7-52):
 *   - extern "C", plain pointers and explicit sizes, no C++/torch types in signatures;
 *   - every function returns int32 status, 0 == success (cpuWolaDll.c:175, cpuToneDll.c:56);
 *   - the CALLER allocates every output (cpuWola.py:60-65); the callee never returns heap memory;
 *   - complex64 is interleaved {float re, float im} (Ipp32fc, cpuWolaDll.c:23);
 *   - stateful objects are create -> use many -> destroy (CyIppXcorrFFT.pyx:25-38).
 * Argument validation with the reference's exception types (TypeError / ValueError /
 * MemoryError) is done by the Python host before the call (cupyHelpers.py:50-82); the
 * library still range-checks everything that could fault the GPU and reports
 * CAF_ERR_INVALID instead of launching.
 *
 * Pointer conventions: names starting with h_ are HOST pointers, d_ are DEVICE (HBM)
 * pointers on the current HIP device.  `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Calls with d_ pointers are asynchronous on `stream`
 * unless stated otherwise; *_host entry points are blocking.  "Asynchronous" is a statement about ordering: all device work of
 * the call is queued on `stream` and nowhere else.  Whether the host returns before that work has run is not promised: an entry
 * point that takes pooled scratch, or that downloads an input to check it, waits for `stream`.  Independence from
 * OTHER streams needs a hardware queue per stream in use at once: HIP maps streams onto GPU_MAX_HW_QUEUES queues (4 by default),
 * and a stream that shares a queue waits behind the other stream's work.  A client that initialises HIP itself sets that variable
 * to cover its streams plus the library's auxiliary ones (one per plan in use, at most 16 kept).
 *
 * Placement: every pointer is aligned to its element type (4 bytes for float32 / int32, 8 for a complex64 or float64 element,
 * 16 for complex128, 2 for int16, 1 for bytes) and nothing more is required unless the entry point says so; a view into a
 * larger array is as good as an allocation of its own.  Results do not depend on where the arrays lie.  Nothing is written
 * outside the outputs, and an argument is read-only unless its entry point says that it is written.
 */
#ifndef CAF_H_
#define CAF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAF_EXPORT __attribute__((visibility("default")))

/* ---- status codes ------------------------------------------------------------------ */
#define CAF_OK 0
#define CAF_ERR_INVALID 1   /* bad argument / shape / range (Python raises ValueError)      */
#define CAF_ERR_HIP 2       /* a HIP runtime call failed (RuntimeError)                      */
#define CAF_ERR_ROCFFT 3    /* a rocFFT call failed (RuntimeError)                           */
#define CAF_ERR_NOMEM 4     /* device or host allocation failed (MemoryError)                */
#define CAF_ERR_NODEVICE 5  /* no usable gfx950 device (RuntimeError)                        */

/* Copies the calling thread's last error message (NUL-terminated) into buf. */
CAF_EXPORT int32_t caf_last_error(char* buf, int32_t len);
/* ABI version of this header: (major << 16) | minor. */
CAF_EXPORT int32_t caf_abi_version(void);

/* ---- device + memory plumbing (replaces cp.asarray / cp.asnumpy / cp.empty at the
 *      cupy-signature entry points, xcorrRoutines.py:81-82,155-156) -------------------- */
CAF_EXPORT int32_t caf_device_count(int32_t* count);
CAF_EXPORT int32_t caf_set_device(int32_t device);
CAF_EXPORT int32_t caf_device_info(int32_t device, char* name, int32_t name_len, int64_t* total_mem,
                                   int32_t* compute_units);
/* caf_malloc / caf_free go through a caching allocator (the counterpart of cupy's default memory pool, which
 * every cp.empty / cp.zeros of the reference's wrappers hits): freed blocks are kept and reused.  A block may be freed
 * while work on the NULL stream still uses it: it is then handed out again only once that work has completed (or to the
 * library's own null-stream scratch, which is ordered behind it), so its next user may sit on any stream.  Work on any
 * other stream must be drained before its blocks are freed;
 * CAF_POOL_MB bounds the cached bytes (default 8192, 0 = plain hipMalloc / hipFree).  caf_pool_trim returns the
 * cache to the driver (cp.get_default_memory_pool().free_all_blocks()).  CAF_POOL_POISON=<32-bit hex word> (diagnostic,
 * read on every allocation; unset, empty or 0 = off) fills every block handed out, reused or fresh, with that word
 * before the allocation returns: outputs and scratch then never start from what an earlier call left in the block. */
CAF_EXPORT int32_t caf_malloc(void** d_ptr, int64_t bytes);
CAF_EXPORT int32_t caf_free(void* d_ptr);
CAF_EXPORT int32_t caf_pool_trim(void);
CAF_EXPORT int32_t caf_pool_stats(int64_t* cached_bytes, int64_t* in_use_bytes, int64_t* hits, int64_t* misses);
CAF_EXPORT int32_t caf_memset(void* d_ptr, int32_t value, int64_t bytes, void* stream);
CAF_EXPORT int32_t caf_h2d(void* d_dst, const void* h_src, int64_t bytes, void* stream);
CAF_EXPORT int32_t caf_d2h(void* h_dst, const void* d_src, int64_t bytes, void* stream);
CAF_EXPORT int32_t caf_d2d(void* d_dst, const void* d_src, int64_t bytes, void* stream);
/* caf_h2d / caf_d2h / caf_d2h_transposed move pageable host memory through the library's own pinned staging buffers
 * (several DMA lanes + host threads for large arrays) and return when the data has arrived: the caller's pages are
 * never registered with the driver, so what the caller does with its arrays afterwards (NumPy returning them to the
 * operating system) cannot stall the process's GPU queues (csrc/caf_host.cpp).
 * caf_d2h_transposed: d_src is [rows][pitch] float32; columns col0 .. col0 + ncols - 1 arrive as the C-ordered host array
 * [ncols][rows] of float32 (dst_f64 = 0) or float64 (1) -- a hypothesis-major surface (caf_outputs2.d_surface_t, rows = F,
 * pitch = S) leaves the device as the (delays, frequencies) array the reference returns (xcorrRoutines.py:553-566,
 * 1028-1039).  rows <= 65536.  (ABI 1.8) */
CAF_EXPORT int32_t caf_d2h_transposed(void* h_dst, int32_t dst_f64, const float* d_src, int64_t rows, int64_t pitch,
                                      int64_t col0, int64_t ncols, void* stream);
/* caf_d2h_f64: count float32 values on the device arrive as float64 on the host (widened by the staging lanes' host threads:
 * the CPU signatures of the reference return float64 surfaces, xcorrRoutines.py:553-566, and NumPy's astype of a 17 GB download
 * is a second pass over it).  (ABI 1.9) */
CAF_EXPORT int32_t caf_d2h_f64(double* h_dst, const float* d_src, int64_t count, void* stream);
CAF_EXPORT int32_t caf_stream_sync(void* stream);
/* a non-blocking HIP stream of the current device for the `stream` arguments below (cupy.cuda.Stream(non_blocking=True)
 * of a cupy caller); NULL = the default stream everywhere */
CAF_EXPORT int32_t caf_stream_create(void** stream);
CAF_EXPORT int32_t caf_stream_destroy(void* stream);

/* ---- the hypothesis engine (frequency-domain overlap-save CAF) -----------------------
 *
 * Computes, for every template t < T, delay s in [shift_start, shift_start+num_shifts) and
 * frequency hypothesis f < F,
 *
 *   QF2[t][s][f] = | sum_n rx[s+n] * conj(tmpl_t[n]) * exp(-j 2 pi nu_f n) |^2
 *                  / ( ||tmpl_t||^2 * sum_{n in supp} |rx[s+n]|^2 )
 *
 * which is the quantity every reference flavour evaluates per delay:
 *   fastXcorr branches A/B/C          xcorrRoutines.py:483-566  (nu_f = k/N, k = FFT bin)
 *   GroupXcorr.xcorr                  xcorrRoutines.py:917-954  (nu_f = freqs[f]/fs, groups)
 *   GroupXcorrFFT.xcorr               xcorrRoutines.py:1137-1189 (nu_f = makeFreq(fftlen)/fs)
 *   cztXcorr / GroupXcorrCZT          xcorrRoutines.py:413-457, 996-1039 (uniform grid)
 *   TemplateCrossCorrelator.correlate xcorrRoutines.py:312-371  (F = 1, T templates)
 *   IppXcorrFFT_32fc::xcorr_thread    cython_ext/CyIppXcorrFFT/IppXcorrFFT.cpp:94-178
 * Instead of one length-N DFT per delay it evaluates one overlap-save correlation per
 * hypothesis: IFFT_B( FFT_B(rx block) * conj(FFT_B(tmpl_t * exp(+j 2 pi nu_f n))) ).
 */
typedef struct caf_plan_t* caf_plan;

/* Frequency-hypothesis specification. */
#define CAF_FREQ_BINS 0  /* nu_f = bins[f] / grid, integer bins (may be negative), grid | block   */
#define CAF_FREQ_NORM 1  /* nu_f = freqs_norm[f] (cycles per sample), arbitrary                  */

typedef struct caf_plan_desc {
    int32_t num_templates;     /* T >= 1                                                          */
    int32_t template_len;      /* N: span of every template in samples (gaps between groups = 0)  */
    const float* h_templates;  /* host, interleaved complex64 [T][N], NOT conjugated              */
    int32_t auto_conj;         /* 1: correlate against conj(template) (reference autoConj=True);  */
                               /* 0: the caller already conjugated                                */
    int32_t num_groups;        /* G >= 1: support = union of [group_start[g], +group_len[g])      */
    const int32_t* h_group_start; /* host [G], relative to the template start; NULL => {0}        */
    const int32_t* h_group_len;   /* host [G]; NULL => {N}                                        */
    int32_t freq_mode;         /* CAF_FREQ_BINS or CAF_FREQ_NORM                                  */
    int32_t num_freqs;         /* F >= 1                                                          */
    const int32_t* h_bins;     /* host [F]  (CAF_FREQ_BINS)                                       */
    int32_t grid;              /* DFT grid size the bins refer to (CAF_FREQ_BINS), e.g. N         */
    const double* h_freqs_norm;/* host [F]  (CAF_FREQ_NORM)                                       */
    int64_t max_rx_len;        /* largest rx length (samples) execute() will be given             */
    int32_t log2_block;        /* overlap-save FFT size B = 2^log2_block; 0 => library default    */
    int32_t blocks_per_batch;  /* rx blocks processed per launch group; 0 => library default      */
    int32_t engine;            /* CAF_ENGINE_AUTO / _ROCFFT / _FUSED / _PERSISTENT / _DIRECT      */
    int32_t reserved;          /* must be 0                                                       */
} caf_plan_desc;

/* Inverse-transform engine of the hypothesis plan.
 *   ROCFFT: spectral multiply kernel -> batched rocFFT inverse -> |.|^2 kernel (any block size);
 *   FUSED : one hand-written kernel does multiply + 16384-point inverse FFT in LDS + |.|^2, a second
 *           one transposes/normalises/argmaxes; needs template_len <= 8192, (bins mode) every
 *           bins[f] * 16384 / grid a whole number (any grid that divides 16384; bin 0 on any grid),
 *           and cannot produce d_cqf.
 *   PERSISTENT: the two FUSED stages as ONE work-queue launch (one resident workgroup per CU): the
 *           HBM-bound transpose runs on some CUs while the others compute FFTs.  Same results as
 *           FUSED up to 8192 samples; templates up to 16384 samples on 32768-point blocks, up to
 *           32768 on 65536-point blocks, up to 262144 on 65536-point blocks with the template cut into
 *           partitions of 32768 samples (bins mode: bins[f] * block / grid whole and even).  d_cqf:
 *           supported as the ONLY output of a call (the FFT work items write the complex rows
 *           themselves, on every block size of this engine).
 *   AUTO  : PERSISTENT when its conditions hold and log2_block is 0 or the engine's own, else ROCFFT. */
#define CAF_ENGINE_AUTO 0
#define CAF_ENGINE_ROCFFT 1
#define CAF_ENGINE_FUSED 2
#define CAF_ENGINE_PERSISTENT 3
/*   DIRECT: the definition itself, product by product in the time domain, for templates with at most 64 non-zero
 *           samples (composite templates whose groups cover only a few samples of a long span): no overlap-save
 *           blocks, so the error does not follow the block's energy; float64 window energies over the samples used.
 *           AUTO picks it for composite templates (num_groups >= 1) whose groups cover fewer than 64 samples.
 *           No d_cqf. */
#define CAF_ENGINE_DIRECT 4

CAF_EXPORT int32_t caf_plan_create(caf_plan* plan, const caf_plan_desc* desc);
CAF_EXPORT int32_t caf_plan_destroy(caf_plan plan);

/* Geometry chosen by the plan: block size B, valid outputs per block, batch, workspace bytes. */
CAF_EXPORT int32_t caf_plan_info(caf_plan plan, int32_t* block, int32_t* step, int32_t* blocks_per_batch,
                                 int64_t* workspace_bytes);

/* Engine actually selected by the plan: CAF_ENGINE_ROCFFT, _FUSED, _PERSISTENT or _DIRECT. */
CAF_EXPORT int32_t caf_plan_engine(caf_plan plan, int32_t* engine);

/* Outputs of one execute (any pointer may be NULL = not wanted).
 * A delay whose rx window holds no energy (a stretch of exact zeros: the reference's 0 / 0) is reported as NaN on the
 * surface and in d_row_max, with d_row_arg = 0, and never becomes a peak. */
typedef struct caf_outputs {
    float* d_surface;      /* [T][num_shifts][F] float32 QF2 (reference CAF layout: delay-major)  */
    float* d_row_max;      /* [T][num_shifts] float32: max over f of QF2                           */
    int32_t* d_row_arg;    /* [T][num_shifts] int32: argmax over f (lowest f on ties)              */
    float* d_peak_val;     /* [T] float32: global maximum of QF2 for template t                    */
    int32_t* d_peak_delay; /* [T] int32: its delay (absolute sample index; lowest on ties)         */
    int32_t* d_peak_freq;  /* [T] int32: its frequency-hypothesis index f                          */
    float* d_cqf;          /* [T][F][num_shifts] complex64 QF = r / (||tmpl|| * ||rx window||), i.e.   */
                           /* hypothesis-major like TemplateCrossCorrelator.correlate (:352-357) and   */
                           /* fastXcorr(absResult=False) (:533-548)                                    */
} caf_outputs;

/* d_rx: device complex64 [rx_len], 8-byte aligned (a whole sample; CAF_ERR_INVALID otherwise).  Requires shift_start >= 0 and
 * shift_start + num_shifts - 1 + N <= rx_len <= max_rx_len.  Asynchronous on `stream`.
 * The plan belongs to the device that was current at caf_plan_create (the same must be current here) and owns
 * its workspace: executions of ONE plan must be ordered (same stream, or synchronised by the caller); different
 * plans may run concurrently from different threads / streams (create -> use many -> destroy, like the
 * reference's stateful correlator objects, IppXcorrFFT.h, xcorrRoutines.py:277-371). */
CAF_EXPORT int32_t caf_plan_execute(caf_plan plan, const float* d_rx, int64_t rx_len, int64_t shift_start,
                                    int64_t num_shifts, const caf_outputs* out, void* stream);

/* The same call with the outputs added after ABI 1.4 (caf_outputs keeps its seven pointers: clients built against it --
 * INTEGRATION.md's ctypes stub, examples/c_client -- stay valid).  `base` as above (may be NULL); zero the struct first. */
typedef struct caf_outputs2 {
    caf_outputs base;
    float* d_surface_t;    /* [T][F][num_shifts] float32 QF2, HYPOTHESIS-major: the same numbers as d_surface, bit for  */
                           /* bit, transposed per template (not the reference's CAF layout, xcorrRoutines.py:553-566;  */
                           /* it is what a frequency-row consumer -- a zoom, a results store, a per-bin detector --     */
                           /* reads contiguously).  Written by the FFT work items of the PERSISTENT engine with        */
                           /* 16384-point blocks themselves: no |y|^2 tiles, no transposition (C2: 10.9 ms against     */
                           /* 13.6).  Not together with d_surface or d_cqf; F == 1: any engine (the layouts coincide). */
    void* reserved[3];     /* must be NULL */
} caf_outputs2;
CAF_EXPORT int32_t caf_plan_execute2(caf_plan plan, const float* d_rx, int64_t rx_len, int64_t shift_start,
                                     int64_t num_shifts, const caf_outputs2* out, void* stream);

/* Diagnostic of the one-launch (persistent) engine: marks[0..1] = the watchdog words of the work-queue block. Both
 * are 0 unless a tile item waited ~10 s for its block to be published -- which the protocol rules out (the launch
 * then traps) -- so a non-zero value after a successful run means a broken hand-off.  Synchronises the device. */
CAF_EXPORT int32_t caf_plan_watchdog(caf_plan plan, int32_t* marks);
/* Per-kernel device timing with HIP events recorded on the execute stream (used by bench.py
 * for the roofline figure).  enable=1 starts collecting; get() synchronises the recorded events
 * and returns accumulated milliseconds and launch counts since enable, per stage:
 *   0 energy prefix+inverse, 1 rx block gather, 2 forward FFT (rocFFT), 3 spectral conj-multiply,
 *   4 inverse FFT (rocFFT), 5 |.|^2 + normalise + argmax, 6 peak reduce.                     */
#define CAF_NUM_STAGES 7
CAF_EXPORT int32_t caf_plan_profile(caf_plan plan, int32_t enable);
CAF_EXPORT int32_t caf_plan_profile_get(caf_plan plan, double* ms /*[CAF_NUM_STAGES]*/,
                                        int64_t* launches /*[CAF_NUM_STAGES]*/);

/* Blocking host-pointer convenience in the reference DLL style (caller-allocated NumPy
 * outputs, host rx): H2D, execute, D2H.  h_* outputs follow caf_outputs shapes. */
CAF_EXPORT int32_t caf_plan_execute_host(caf_plan plan, const float* h_rx, int64_t rx_len, int64_t shift_start,
                                         int64_t num_shifts, float* h_surface, float* h_row_max,
                                         int32_t* h_row_arg, float* h_peak_val, int32_t* h_peak_delay,
                                         int32_t* h_peak_freq);

/* ---- the per-delay path (one DFT per delay; what the reference literally does) --------------
 *
 * For delays s_i = start + i*step, i < num:   z_i = FFT_N( rx[s_i : s_i+N] * cutout ) / (||cutout|| ||rx window||)
 * replaces fastXcorr branches B/B'/C/C' (xcorrRoutines.py:511-580), cp_fastXcorr (:29-167) and
 * IppXcorrFFT_32fc::xcorr_thread (IppXcorrFFT.cpp:94-178).  `d_cutout` is used AS GIVEN (the caller
 * passes conj(cutout) for the usual correlation, like ippsMul_32fc(m_cutout(conj'd), ...) :133-138).
 * Outputs (any may be NULL): d_qf2[num] = max_k |z_i[k]|^2, d_fidx[num] = first argmax bin,
 * d_caf[num][N] = |z_i|^2 (float32), d_ccaf[num][N] = z_i (complex64).
 * zero_oor != 0: delays whose window leaves [0, rx_len) give (0, 0) / zero rows (IppXcorrFFT.cpp:125-130);
 * zero_oor == 0: such a delay is an error (CAF_ERR_INVALID). Blocking (allocates and frees scratch).
 * Zero-energy windows (a stretch of exact zeros in rx under the whole cutout -- the reference's 0 / 0,
 * `pmax / cutoutNormSq / rxNormPartSq`, xcorrRoutines.py:527-528; IppXcorrFFT.cpp:174): d_qf2 = NaN, d_fidx = 0, NaN rows in
 * d_caf / d_ccaf -- the same rule as caf_outputs.d_row_max / d_row_arg above.  (Only the stand-alone
 * caf_argmax_abs_rows keeps the (0, 0) of the CUDA kernel's zero-initialised workspace, argmax.cu:108-109.) */
CAF_EXPORT int32_t caf_xcorr_perdelay(const float* d_cutout, int32_t n, const float* d_rx, int64_t rx_len,
                                      int64_t start, int64_t step, int64_t num, int32_t zero_oor, float* d_qf2,
                                      int32_t* d_fidx, float* d_caf, float* d_ccaf, int64_t batch_rows, void* stream);
/* Cutouts of 32 .. 16384 samples whose prime factors are at most 23 get a kernel compiled for the length at run time (hiprtc, as the reference
 * compiles its own through NVRTC; cached in memory and under CAF_JIT_CACHE / ~/.cache/pydsproutines_amd/jit; CAF_JIT=0 keeps the
 * prebuilt kernels).  This call describes what would run for n -- radices, threads per row, LDS strides, the bank-conflict
 * cycles its layout was chosen by -- as one line of text in buf ("" when the length has no such kernel), without a GPU.
 * arch != NULL (e.g. "gfx950"): the kernel is also compiled (not loaded); dump_path != NULL: its code object is written there.
 * (ABI 1.8) */
CAF_EXPORT int32_t caf_perdelay_jit_describe(int32_t n, const char* arch, const char* dump_path, char* buf, int32_t len);
/* 1 when caf_xcorr_perdelay serves cutouts of n samples with ONE kernel (product, N-point transform in LDS, |.|^2, argmax:
 * powers of two 64 ... 16384, 100 / 1000 / 10000, and the 2^a 3^b 5^c 7^d lengths 32 ... 16200 the mixed-radix planner
 * finds a plan for), 0 when it runs the product rows -> row FFT -> argmax chain the reference runs for every length
 * (cp_fastXcorr_v2, xcorrRoutines.py:169-274).  The results are the same either way; callers that batch the chain
 * themselves (the BATCH argument of cp_fastXcorr_v2) ask this first.  No device work. */
CAF_EXPORT int32_t caf_xcorr_perdelay_one_kernel(int32_t n);

/* ---- stand-alone kernels (device pointers), one per reference CUDA kernel wrapper ------------- */
/* batched row FFT, replaces cp.fft.fft(x, axis=1) / ifft (xcorrRoutines.py:135,246,339,352); in place when
 * d_out == d_in; inverse != 0 applies the 1/len normalisation of numpy/cupy ifft. */
CAF_EXPORT int32_t caf_fft_rows(const float* d_in, float* d_out, int64_t rows, int64_t len, int32_t inverse,
                                void* stream);
/* slidingMultiplyNormalised (multiplySlices.cu:113-216, cupyExtensions.py:491-560): d_z[idxlen][xlen] */
CAF_EXPORT int32_t caf_sliding_multiply_normalised(const float* d_x, int32_t xlen, const float* d_y, int64_t ylen,
                                                   int64_t start_idx, int64_t idxlen, double coefficient,
                                                   float* d_z, void* stream);
/* multiTemplateSlidingDotProduct (multiplySlices.cu:251-399, cupyExtensions.py:563-640) */
CAF_EXPORT int32_t caf_multi_template_sliding_dot(const float* d_templates, const float* d_energies, int32_t num_templates,
                                                  int32_t template_len, const float* d_x, int64_t xlen,
                                                  int64_t start_idx, int64_t idxlen, int32_t* d_template_idx,
                                                  float* d_qf2, void* stream);
/* multiplySlicesWithIndexedRowsOptimistic (multiplySlices.cu:25-84, cupyExtensions.py:405-488) */
/* d_out[num_slices][out_len]; slice i covers d_slice_lens[i] samples (NULL = out_len), zero beyond */
CAF_EXPORT int32_t caf_multiply_slices_indexed_rows(const float* d_x, int64_t xlen, const float* d_rows, int32_t num_rows,
                                                    int32_t row_len, const int32_t* d_slice_starts,
                                                    const int32_t* d_slice_lens, const int32_t* d_row_idx,
                                                    int32_t out_len, int64_t num_slices, float* d_out, void* stream);
/* complex_magnSq_kernel<T,U> (complex_magn.cu:8-19): in complex64 (in_c128=0) or complex128, out f32 or f64 */
CAF_EXPORT int32_t caf_complex_magnsq(const void* d_x, int64_t n, int32_t in_c128, void* d_out, int32_t out_f64,
                                      void* stream);
/* multiArgmaxAbsRows_complex64 (argmax.cu:93-153): first index of the maximum (NumPy tie-break) */
CAF_EXPORT int32_t caf_argmax_abs_rows(const float* d_x, int64_t rows, int64_t len, uint32_t* d_argmax, float* d_max,
                                       int32_t use_normsq, void* stream);
/* movingAverage (filter.cu:291-347), multiMovingAverage (:196-240): causal, zero history, per row */
CAF_EXPORT int32_t caf_moving_average(const float* d_x, int64_t rows, int64_t n, int32_t avg_length,
                                      int32_t sum_instead, float* d_out, void* stream);
/* movingComplexSum (filter.cu:374-438): d_out[n - L + 1] = |sum of L consecutive samples|^2 */
CAF_EXPORT int32_t caf_complex_moving_sum(const float* d_x, int64_t n, int32_t sum_length, float* d_out, void* stream);
/* copy*SlicesToMatrix_32fc (copying.cu:8-138): row i = x[starts[i] : +len] (starts_stride 1), the
 * [start,end) rows of an (N,2) bounds array (starts_stride 2, zero beyond end), or x[start0 + i*inc : +len]
 * when d_starts is NULL; samples outside x read as 0 */
CAF_EXPORT int32_t caf_copy_slices_to_matrix(const float* d_x, int64_t xlen, const int32_t* d_starts,
                                             int32_t starts_stride, int64_t start0, int64_t increment, int32_t len,
                                             int64_t rows, float* d_out, void* stream);
/* copy_groups_kernel32fc (cupyExtensions.py:17-38): d_y[d_y_starts[g] : + d_lengths[g]] = d_x[d_x_starts[g] : + d_lengths[g]] for
 * every group g; d_y is written there and keeps what it held everywhere else */
CAF_EXPORT int32_t caf_copy_groups(const float* d_x, float* d_y, const int32_t* d_x_starts, const int32_t* d_y_starts,
                                   const int32_t* d_lengths, int32_t num_groups, void* stream);
/* findLocalMaxima (peakfinding.cu:14-58): indices in ASCENDING order (deterministic), *d_count = total found */
CAF_EXPORT int32_t caf_find_local_maxima(const float* d_x, int64_t n, float min_height, int32_t max_peaks,
                                         int32_t* d_peak_index, int32_t* d_count, void* stream);
/* d_out[i] = d_x[d_index[i]] for 4-byte elements (float32 / int32; 0 for indices outside [0, xlen)): the values and
 * frequency arguments at the candidate peaks without copying whole per-delay traces to the host (the fancy
 * indexing d_trace[d_idx] of a cupy caller after cupyFindLocalMaxima, cupyExtensions.py:651-686) */
CAF_EXPORT int32_t caf_gather_b32(const void* d_x, int64_t xlen, const int32_t* d_index, int64_t n, void* d_out,
                                  void* stream);
/* ---- multi-GPU step --------------------------------------------------------------------------------
 * One process per GPU; templates are block-sharded over the ranks, rx is replicated, and the only exchange of the
 * path is the all-gather of the per-template peak rows over RCCL / xGMI.  Rank 0 obtains a 128-byte id and hands it
 * to the other ranks through any host channel (MPI, a file, torch.distributed's store); every rank then creates the
 * communicator with its GPU current.  d_local = this rank's rows as [3][rows_per_rank] int32 (delays, frequency
 * indices, float32 peak values as bits: the three d_peak_* arrays of caf_outputs laid end to end, shards padded to
 * the largest); d_table = [world][3][rows_per_rank], identical on every rank.  The reference has no multi-GPU code;
 * its nearest analogue is the thread-strided split of cython_ext/CyIppXcorrFFT/IppXcorrFFT.cpp:117. */
typedef struct caf_comm_t* caf_comm;
CAF_EXPORT int32_t caf_comm_unique_id(void* id128);
CAF_EXPORT int32_t caf_comm_create(caf_comm* comm, int32_t world_size, int32_t rank, const void* id128);
CAF_EXPORT int32_t caf_comm_destroy(caf_comm comm);
CAF_EXPORT int32_t caf_peak_table_allgather(caf_comm comm, const int32_t* d_local, int32_t rows_per_rank,
                                            int32_t* d_table, void* stream);

/* d_out[i] = (double) d_x[d_index ? d_index[i] : i] (0 outside [0, xlen)): float32 per-delay traces into the float64
 * device arrays the reference's GPU entry points return (GroupXcorrFFT.xcorrGPU xc = cp.zeros(shifts.size),
 * xcorrRoutines.py:1198-1203; cp_fastXcorr's d_result, :95-101) with no host round trip */
CAF_EXPORT int32_t caf_gather_f32_f64(const float* d_x, int64_t xlen, const int32_t* d_index, int64_t n, double* d_out,
                                      void* stream);
/* ---- config C5 in one call: coarse CAF -> top-k local maxima -> chirp-Z fine zoom ------------------------------
 * Replaces the reference's two-stage workflow of a coarse xcorr followed by a CZT over a narrow span at the delays of
 * interest (benchmarks/benchmark_czts.py:31-82 with pbIppCZT32fc.runMany; cztXcorr xcorrRoutines.py:413-457;
 * pybinds/ippGroupXcorrCZT/GroupXcorrCZT.cpp:202-329).  Input: the per-delay trace of ONE template of a finished
 * caf_plan_execute (d_row_max / d_row_arg offset to that template, num_shifts entries starting at shift_start).
 * On the device: local maxima above min_height (peakfinding.cu:52 predicate) -> the k strongest (value descending,
 * delay ascending) -> per peak the normalised product row rx[d:d+N] * conj(template) -> |CZT|^2 on the grid
 * nu0 - span ... nu0 + span in steps of `step` (all in cycles per sample; nu0 = the peak's coarse frequency).
 * Every output is a caller-allocated DEVICE array with k entries (NULL to skip); unused entries have delay -1.
 * d_count[0] = peaks returned (<= k), or -1 when more than 2^20 local maxima exceed min_height (raise it). */
typedef struct caf_zoom_outputs {
    int32_t* d_count;              /* [1] */
    int32_t* d_delay;              /* [k] absolute delay index */
    int32_t* d_coarse_freq_index;  /* [k] hypothesis index of the coarse maximum at that delay */
    float* d_coarse_qf2;           /* [k] */
    int32_t* d_fine_index;         /* [k] argmax on the fine grid (first index) */
    double* d_fine_freq;           /* [k] its frequency, cycles per sample: nu0 - span + index * step */
    float* d_fine_qf2;             /* [k] */
    float* d_planes;               /* [k][num_bins] fine |CZT|^2 (num_bins from caf_zoom_num_bins) */
} caf_zoom_outputs;
CAF_EXPORT int32_t caf_zoom_num_bins(double span, double step, int32_t* num_bins);
CAF_EXPORT int32_t caf_zoom_czt(caf_plan plan, int32_t template_index, const float* d_rx, int64_t rx_len,
                                const float* d_row_max, const int32_t* d_row_arg, int64_t shift_start, int64_t num_shifts,
                                int32_t k, float min_height, double span, double step, const caf_zoom_outputs* out,
                                void* stream);

/* filter_smtaps* (filter.cu:9-181) == scipy.signal.lfilter(taps, 1, x)[ds_phase::dsr] with carried-in history */
CAF_EXPORT int32_t caf_fir_lfilter(const float* d_x, int64_t n, const float* d_taps, int32_t num_taps,
                                   const float* d_delay, int32_t delay_len, int32_t dsr, int32_t ds_phase, float* d_out,
                                   int64_t out_len, void* stream);
/* WOLA polyphase channeliser: filterRoutines.wola (filterRoutines.py:578-632), cpuWola.cpu_threaded_wola
 * (cpuWola.py:19-70 over cpuWolaDll.c:38-178) and the history of filterRoutines.Channeliser (filterRoutines.py:636-690).
 * Input = the hist_len complex64 samples of d_hist (carried-in history, NULL/0 for none) followed by the n samples of d_x;
 * output row r < rows (rows <= n / dec) is taken at d_x[r * dec]:
 *   v[a] = sum_{b < L/N} d_taps[b N + a] * input[r dec - b N - a]   (zero before the history),  a < N = num_channels
 *   out[r][k] = sum_a v[a] e^{+j 2 pi a k / N}                        (no 1/N), negated at odd k on odd r when N == 2 dec.
 * num_channels must be dec or 2 * dec and num_taps (L) a multiple of it.  layout 0: d_out is (rows, N) time-major (the
 * reference's); 1: (N, rows) channel-major, one channel a contiguous rx.  N a power of two 64..16384 with L/N <= 64 runs
 * one fused kernel; anything else runs polyphase sums + batched rocFFT rows (CAF_WOLA_FUSED=0 forces that).  (ABI 1.10) */
CAF_EXPORT int32_t caf_wola(const float* d_x, int64_t n, const float* d_hist, int64_t hist_len, const float* d_taps,
                            int64_t num_taps, int32_t num_channels, int32_t dec, int32_t layout, float* d_out, int64_t rows,
                            void* stream);
/* ---- burst detection (filterRoutines.py:701-1088, thresholding.cu:27-225).  Added after ABI 1.10 without a version bump:
 * clients detect these entry points by symbol.  dtype / is_f64 select float32 (0) or float64 (1) real input. ---- */
/* BurstDetector.medfilt (:805-819): d_abs = |x| (hypot for complex), d_ampsq = d_abs * d_abs in the same precision
 * (not re^2 + im^2).  dtype 0 complex64 -> float32, 1 complex128 -> float64, 2 float32, 3 float64 (abs only). */
CAF_EXPORT int32_t caf_abs_ampsq(const void* d_x, int64_t n, int32_t dtype, void* d_abs, void* d_ampsq, void* stream);
/* cupyx.scipy.signal.medfilt as called by BurstDetector.medfilt / energyDetection (:819, :1073): d_out[i] = the order
 * statistic kernel_size / 2 of x[i - W/2 .. i + W/2], samples outside [0, n) counted as +0.0 (== scipy.signal.medfilt).
 * kernel_size odd >= 1, may exceed n.  Small windows select in registers; larger ones (or CAF_MEDFILT_GENERAL=1) query a
 * wavelet matrix built in pool scratch. */
CAF_EXPORT int32_t caf_medfilt(const void* d_x, int64_t n, int32_t is_f64, int64_t kernel_size, void* d_out, void* stream);
/* thresholdEdges (thresholding.cu:27-156) in the reference's layout: B = threads_per_block - 2, rows = ceil(n / B);
 * sample i >= 1 belongs to row (i - 1) / B; m[j] = x[j] > threshold, m[n] = 0; +i for a left edge (m[i] && !m[i-1] &&
 * m[i+1]), -i for a right edge (m[i] && m[i-1] && !m[i+1]).  d_edges (rows, edges_max): each row's first edges_max edges
 * in ascending order, then zeros; d_counts[row] = the row's true count.  3 <= threads_per_block <= 1024, n < 2^31. */
CAF_EXPORT int32_t caf_threshold_edges(const float* d_x, int64_t n, float threshold, int32_t threads_per_block,
                                       int32_t edges_max, int32_t* d_edges, int32_t* d_counts, void* stream);
/* gatherThresholdEdgesResults (thresholding.cu:159-225): the stored edges of rows with a non-zero count (the first
 * min(count, edges_max) entries, zeros skipped), row-major, through the pairing state machine (left = 0; a left edge sets
 * left; a right edge R emits (left, R) when min_len <= R - left <= max_len and resets left to 0).  Writes the first
 * min(K, capacity) int32 pairs to d_pairs[K][2]; *h_num_pairs = K (host).  Synchronises the stream. */
CAF_EXPORT int32_t caf_gather_edges(const int32_t* d_edges, int64_t rows, int32_t edges_max, const int32_t* d_counts,
                                    int32_t min_len, int32_t max_len, int32_t* d_pairs, int64_t capacity,
                                    int64_t* h_num_pairs, void* stream);
/* BurstDetector.detectViaThreshold (:843-852): the K int64 indices with x > threshold (threshold cast to the array's
 * dtype) and, for each of the R maximal runs of consecutive indices, the position in that index array where it starts.
 * h_counts[0] = K, h_counts[1] = R (host).  d_idx == NULL: counts only.  Synchronises the stream. */
CAF_EXPORT int32_t caf_threshold_indices(const void* d_x, int64_t n, int32_t is_f64, double threshold, int64_t* d_idx,
                                         int64_t idx_cap, int64_t* d_run_starts, int64_t runs_cap, int64_t* h_counts,
                                         void* stream);
/* cp.histogram(x, edges)[0] of autoDetectThreshold (:911) == np.histogram: bins [e_i, e_i+1), the last one closed,
 * compared in float64; values outside the edges and NaN are not counted.  d_edges increasing, num_edges >= 2;
 * d_counts int64[num_edges - 1]. */
CAF_EXPORT int32_t caf_histogram(const void* d_x, int64_t n, int32_t is_f64, const double* d_edges, int64_t num_edges,
                                 int64_t* d_counts, void* stream);
/* the column means of detectRegularSections (:964-967): d_out[c] = mean_r (absolute ? |x[r][c]| : x[r][c]) of a
 * (rows, cols) matrix, accumulated in float64. */
CAF_EXPORT int32_t caf_column_means(const void* d_x, int64_t rows, int64_t cols, int32_t is_f64, int32_t absolute,
                                    double* d_out, void* stream);
/* upfirdn_naive / upfirdn_sm (upfirdn.cu:6-182) == scipy.signal.upfirdn(taps, x, up, down) per row */
CAF_EXPORT int32_t caf_upfirdn(const float* d_x, int64_t rows, int64_t n, const float* d_taps, int32_t num_taps,
                               int32_t up, int32_t down, float* d_out, float* d_out_abs, int64_t out_len, void* stream);
/* CZTCachedGPU.runMany (spectralRoutines.py:370-391) / IppCZT32fc::runMany (CZT.cpp): rows of length m ->
 * k CZT bins; aa[m], fv[nfft], ww_slice[k] are the cached complex64 constants (host computes them in f64). */
CAF_EXPORT int32_t caf_czt_run_many(const float* d_x, int64_t rows, int32_t m, int32_t k, int32_t nfft,
                                    const float* d_aa, const float* d_fv, const float* d_ww, float* d_out,
                                    void* stream);
/* multiArgmax3d_uint32 (argmax.cu:11-81, cupyExtensions.py:225-265): per item of a (items, d1, d2, d3) uint32
 * array, the three indices of its maximum (first flat index on ties) -> d_argmax[items][3], d_max[items] */
CAF_EXPORT int32_t caf_argmax3d_u32(const uint32_t* d_x, int64_t num_items, int32_t dim1, int32_t dim2, int32_t dim3,
                                    uint32_t* d_argmax, uint32_t* d_max, void* stream);
/* IQ ingest: interleaved int16 I/Q -> complex64 * scale on the device, i.e. the
 * np.fromfile(int16).astype(float32).view(complex64) of usrpRoutines.simpleBinRead (usrpRoutines.py:51-67)
 * done after the (half-size) H2D copy as in benchmarks/benchmark_cupyCopyAndConvert.py:17-25.
 * d_iq must be 8-byte and d_out 16-byte aligned (two samples a load, two a store; CAF_ERR_INVALID otherwise). */
CAF_EXPORT int32_t caf_iq16_to_c64(const int16_t* d_iq, int64_t num_samples, float scale, float* d_out, void* stream);
/* Front-end filter/decimate fused into the rx load: one kernel that is
 *   caf_iq16_to_c64 -> filter_smtaps(dsr, dsPhase)   (usrpRoutines.py:51-67 + filter.cu:9-58, filterRoutines.py:417-501)
 * i.e. d_out[o] = lfilter(taps, 1, scale * iq)[ds_phase + o*dsr] as complex64, reading the raw int16 pairs (4 B per
 * input sample) and computing only the kept outputs.  d_delay = the delay_len int16 IQ pairs that precede d_iq
 * (streaming state: the tail of the previous chunk), NULL/0 for zeros.  num_taps <= 2048, dsr <= 16.
 * d_iq and d_delay must be 4-byte aligned (a whole IQ pair; CAF_ERR_INVALID otherwise). */
CAF_EXPORT int32_t caf_iq16_fir_decimate(const int16_t* d_iq, int64_t num_samples, float scale, const float* d_taps,
                                         int32_t num_taps, const int16_t* d_delay, int32_t delay_len, int32_t dsr,
                                         int32_t ds_phase, float* d_out, int64_t out_len, void* stream);
/* per column of a complex64 (rows, n) matrix: max_r |z| and the first row attaining it
 * (TemplateCrossCorrelator.correlate(returnMax=True), xcorrRoutines.py:361-371) */
CAF_EXPORT int32_t caf_colmax_abs(const float* d_z, int32_t rows, int64_t n, float* d_max, void* d_arg,
                                  int32_t arg_int64 /* d_arg is int64[n] (cp.argmax's dtype) instead of int32[n] */, void* stream);
/* the same reduction on per-template QF^2 traces (float32 (rows, n), e.g. caf_outputs.d_row_max of an F = 1 plan):
 * d_max[i] = max_r sqrt(q2[r][i]), d_arg[i] = its first row as int64 (the dtype cp.argmax returns) */
CAF_EXPORT int32_t caf_colmax_sqrt(const float* d_q2, int32_t rows, int64_t n, float* d_max, int64_t* d_arg, void* stream);
/* Tone-dot zoom, dotTonesScaling_32f (genTones.cu:165-283, cupyDotTonesScaling spectralRoutines.py:580-630):
 * d_out[b][k] (complex64, ceil(len/64) x num_freqs) = sum over the 64-sample block b of
 * d_src[i] * exp(j 2 pi (f0 + k fstep) i), f0 / fstep normalised (cycles per sample); summing over b gives the
 * CZT of d_src at the normalised frequencies -(f0 + k fstep) */
CAF_EXPORT int32_t caf_dot_tones(const float* d_src, int64_t len, double f0, double fstep, int32_t num_freqs,
                                 float* d_out, void* stream);
/* Sub-sample refinement after the peak (fineFreqTimeSearch / GenXcorr.xcorr, xcorrRoutines.py:583-719):
 * d_out[i] = d_a[i] * conj(d_b[i]) (complex64; `x_fft * y_fft.conj()` :648, `y_aligned.conj() * x_aligned` :622) */
CAF_EXPORT int32_t caf_mul_conj(const float* d_a, const float* d_b, int64_t n, float* d_out, void* stream);
/* d_out[r] (complex128) = scale * sum_k d_vec[k] (complex64) * conj(d_steer[r][k]) (complex128 [rows][n]):
 * `np.dot(rx_vec, steeringvec.conj().T) / norms` :661-665, `np.vdot(precomputed, fineshifts[j])` :630 */
CAF_EXPORT int32_t caf_steer_dot(const float* d_vec, const double* d_steer, int64_t rows, int64_t n, double scale,
                                 double* d_out, void* stream);
/* GroupXcorrCZT_Permutations.getCAF / getCAF_GPU (xcorrRoutines.py:1454-1484, 1549-1585): sum the selected
 * per-template complex64 planes d_planes[num_planes][rows][cols] (h_sel: host array of num_sel <= 64 plane
 * numbers), then d_out[rows][cols] (float64) = |sum|^2 / d_row_norm[row] (float64) / ynormsq */
CAF_EXPORT int32_t caf_sum_planes_qf2(const float* d_planes, int32_t num_planes, int64_t rows, int32_t cols,
                                      const int32_t* h_sel, int32_t num_sel, const double* d_row_norm, double ynormsq,
                                      double* d_out, void* stream);
/* The coherent sum over the groups of ONE composite template on the per-delay path (GroupXcorrCZT.xcorr,
 * xcorrRoutines.py:996-1039; GroupXcorrCZT.cpp:106-329): d_planes[num_groups][rows][cols] complex64 = the chirp-Z rows of
 * every group's products as if the group began at sample 0, d_phase[num_groups][cols] complex64 = e^{-j 2 pi f_col start_g / fs}
 * (NULL: all ones); d_out[rows][cols] (float64) = |sum_g phase planes|^2 / d_row_norm[row] / ynormsq.  Any number of groups. */
CAF_EXPORT int32_t caf_sum_groups_qf2(const float* d_planes, int32_t num_groups, int64_t rows, int32_t cols,
                                      const float* d_phase, const double* d_row_norm, double ynormsq, double* d_out,
                                      void* stream);

/* ---- PSK demodulation of bursts (demodulationRoutines.py:44-590, 626-1206; custom_kernels/demodulation.cu, eyeOpeningKernel.cu) --
 * One row = one burst, zero-padded to the matrix width.  Sums are float32 in a fixed order that depends on the row alone. */
#define CAF_DEMOD_LOCK_EIG 0       /* leading eigenvector of the 2x2 moment matrix of x^(m/2) (lockPhase)           */
#define CAF_DEMOD_LOCK_POWERSUM 1  /* arg(sum x^m) / m (demod_qpsk, demod_b_or_q_psk)                                  */
#define CAF_DEMOD_LOCK_NONE 2      /* no rotation at all: the row is mapped as it is (mapSyms alone)                   */
#define CAF_DEMOD_MAP_CLASS 0      /* SimpleDemodulatorBPSK / QPSK / 8PSK.mapSyms (comparisons with 0; QPSK at +pi/4)  */
#define CAF_DEMOD_MAP_GENERIC 1    /* SimpleDemodulatorPSK.mapSyms: arg max of the dot product with pskdicts[m]        */
#define CAF_DEMOD_MAP_SIGNBITS 2   /* demod_qpsk / demod_b_or_q_psk: anticlockwise 0..3 from the sign bits             */
#define CAF_DEMOD_MAP_GRAYBATCH 3  /* lockPhase_mapSyms_singleBlkKernel_qpsk: ((re >= +0) << 1) | (im >= +0)           */
typedef struct caf_demod_desc {
    const float* d_x;        /* (rows, xlength) complex64                                                             */
    int64_t rows, xlength;
    int32_t osr;             /* samples per symbol, 1..32; a row has xlength / osr symbols                            */
    int32_t m;               /* 2, 4 or 8 for every row, unless d_m is given                                          */
    const uint8_t* d_m;      /* NULL or rows orders; a row whose order is not 2 / 4 / 8 is left untouched             */
    const int32_t* d_lengths;/* NULL or the valid samples of each row (the rest of the row is padding)                */
    const float* d_abs;      /* NULL or |x| (rows, xlength); when NULL |x| is formed in the kernel                    */
    int32_t lock, map;       /* CAF_DEMOD_LOCK_*, CAF_DEMOD_MAP_*                                                     */
    uint8_t* d_syms;         /* (rows, xlength / osr)                                                                 */
    int32_t* d_eo_index;     /* optional outputs from here on: rows                                                   */
    float* d_eo_metric;      /* (rows, osr): the SUM of |x| of every phase                                            */
    float* d_angle;          /* rows: the eigenvector's angle, or arg(sum x^m)                                        */
    float* d_svd;            /* rows: lambda2 / lambda1 (eigen form)                                                  */
    float* d_moments;        /* (rows, 3): S00, S01, S11 (eigen form) or Re, Im of the power sum and 0                */
    float* d_reimc;          /* (rows, xlength / osr) complex64: the rotated symbols                                  */
    float* d_xeo;            /* (rows, xeo_pitch) complex64: the winning phase, copied                                */
    int64_t xeo_pitch;
    int32_t eye_only;        /* (set by caf_eye_opening_batch)                                                        */
    int32_t num_preambles;   /* 0: no preamble stage                                                                  */
    const uint8_t* d_preambles;          /* the preambles, concatenated (preamble_total bytes)                        */
    const int32_t* d_preamble_lengths;   /* num_preambles lengths                                                     */
    int32_t preamble_total, max_preamble_length;
    int32_t search_start, search_end;
    uint32_t* d_best;        /* (rows, 4): preamble, sample (search_start + index), rotation, matches                 */
    uint8_t* d_payload;      /* (rows, out_length): gray[(sym + rotation) mod m] from sample + preamble length        */
    uint32_t* d_count;       /* rows: symbols in the row after the preamble (NULL: not wanted)                        */
    int64_t out_length;
    float scaling;           /* > 0: max(eo_metric) of the 8PSK threshold (mapSyms alone); 0: this row's own eye-opening mean */
    int32_t reserved;
} caf_demod_desc;
/* eye opening -> phase lock -> symbol map, and with preambles compare -> arg max -> cut / rotate / gray, in ONE launch.
 * 8PSK rows skip the preamble stage (no gray map is defined for them).  (ABI 1.10, detected by symbol) */
CAF_EXPORT int32_t caf_psk_demod_rows(const caf_demod_desc* desc, void* stream);
/* getEyeOpening_batch (eyeOpeningKernel.cu:5-83): d_abs may be NULL; d_eo_index / d_eo_metric (rows, osr sums) optional */
CAF_EXPORT int32_t caf_eye_opening_batch(const float* d_abs, const float* d_x, int64_t rows, int64_t xlength, int32_t osr,
                                         float* d_xeo, int64_t xeo_pitch, int32_t* d_eo_index, float* d_eo_metric, void* stream);
/* compareIntegerPreambles (demodulation.cu:547-661): d_matches[row][preamble][search][r] (uint32) = the number of j with
 * (preamble[j] - syms[search_start + search + j]) mod m == r; rows whose d_psk_m (optional) differs from m are not written */
CAF_EXPORT int32_t caf_compare_int_preambles(const uint8_t* d_syms, int64_t rows, int64_t syms_length, int32_t search_start,
                                             int32_t search_end, const uint8_t* d_preambles, int32_t preamble_total,
                                             const int32_t* d_preamble_lengths, int32_t num_preambles,
                                             int32_t max_preamble_length, int32_t m, const uint8_t* d_psk_m,
                                             uint32_t* d_matches, void* stream);
/* cutAndRotatePSKSymbolsFromPossiblePreambles_Gray (demodulation.cu:41-115): d_index (rows, 3) = key, sample, rotation */
CAF_EXPORT int32_t caf_cut_rotate_gray(const uint32_t* d_index, int64_t rows, const uint8_t* d_syms, int64_t syms_length,
                                       const uint32_t* d_key_lengths, int32_t num_keys, const uint32_t* d_sample_stops,
                                       int32_t m, int64_t out_length, uint8_t* d_out, uint32_t* d_count,
                                       const uint8_t* d_psk_m, void* stream);
/* the amble search and bit unpacking of lockPhase_mapSyms_singleBlkKernel_qpsk (demodulation.cu:985-1088) on the uint8
 * gray symbols of caf_psk_demod_rows(CAF_DEMOD_MAP_GRAYBATCH); d_amble is int32 as in the reference */
CAF_EXPORT int32_t caf_amble_search_bits(const uint8_t* d_syms, int64_t rows, int64_t syms_length, const int32_t* d_amble,
                                         int32_t amble_length, int32_t search_start, int32_t search_length,
                                         uint32_t* d_syms_out, int32_t* d_best_matches, int32_t* d_best_rotations,
                                         int32_t* d_best_idx, uint8_t* d_bits, int64_t bits_length, void* stream);

/* ---- CP2FSK demodulation (demodulationRoutines.py:20-37, 1214-1330).  Added after ABI 1.10 without a version bump, detected by
 * symbol.  With g[n] = exp(j pi h n / up), n < up (float64, rounded once to float32), for a position i of a row:
 *   c0[i] = |sum_n x[i + n] g[n]|, c1[i] = |sum_n x[i + n] conj(g[n])|, bit[i] = (c1[i] > c0[i]), m[i] = max(c0[i], c1[i])
 * (float32 sums in a fixed order).  1 <= up <= 256.  No argument combination reaches outside a row: what does not fit is
 * refused with CAF_ERR_INVALID before anything is launched. */
/* the positions i = start + k step, k < count, of every row of d_x (rows, xlength) complex64: step = 1 slides, step = up walks
 * symbol by symbol.  d_c0, d_c1, d_max (rows, count) float32 and d_bits (rows, count) uint8; any of them may be NULL. */
CAF_EXPORT int32_t caf_cp2fsk_tone_metric(const float* d_x, int64_t rows, int64_t xlength, int32_t up, double h, int64_t start,
                                          int64_t step, int64_t count, float* d_c0, float* d_c1, float* d_max, uint8_t* d_bits,
                                          void* stream);
/* d_costs[row][k] (float64) = sum_b sum_{j < burst_len} d_max[row][search_start + k + burst_starts[b] + j up], k < search_count.
 * burst_starts is a HOST array of num_bursts sample offsets >= 0 (up to 128 of them travel with the launch; a longer list is
 * uploaded first, which waits for the stream once). */
CAF_EXPORT int32_t caf_cp2fsk_comb_costs(const float* d_max, int64_t rows, int64_t mlength, int32_t up, int32_t burst_len,
                                         const int64_t* burst_starts, int32_t num_bursts, int64_t search_start,
                                         int64_t search_count, double* d_costs, void* stream);
/* BurstyDemodulatorCP2FSK.demod of every row: sliding metrics, costs of the search range, d_mi[row] (int64) = search_start + the
 * first arg max of the row's costs, d_dbits (rows, num_bursts burst_len) uint8 = bit[mi + burst_starts[b] + j up];
 * d_costs (rows, search_count) float64 is optional. */
CAF_EXPORT int32_t caf_cp2fsk_bursty_demod(const float* d_x, int64_t rows, int64_t xlength, int32_t up, double h, int32_t burst_len,
                                           const int64_t* burst_starts, int32_t num_bursts, int64_t search_start,
                                           int64_t search_count, int64_t* d_mi, uint8_t* d_dbits, double* d_costs, void* stream);

/* ---- TDOA / FDOA grid-search geolocation (localizationRoutines.py:510-748, 1380-1511).  Added after ABI 1.10 without a version
 * bump, detected by symbol.  Everything is float64.  For a grid point p and a measurement record (s1, s2, v1, v2, r, wr, d, wd):
 *   rho1 = |p - s1|, rho2 = |p - s2|, e = r - (rho2 - rho1), f = d - ((p - s2).v2 / rho2 - (p - s1).v1 / rho1),
 *   cost[p] = sum_k (wr_k e_k^2 + wd_k f_k^2), in the order of k, the TD term before the FD term of the same k.
 * The library knows nothing of seconds, hertz or carrier frequencies: r and d are a range difference and a range-rate
 * difference, wr and wd their weights. */
#define CAF_LOCATE_POINTS 0   /* d_points: an (n, 3) matrix of points                                               */
#define CAF_LOCATE_MESH 1     /* p(i, j) = (A[i] C[j], A[i] S[j], Z[i]), flat index i nj + j; never materialised     */
#define CAF_LOCATE_MESH_XY 2  /* p(i, j) = (X[j], Y[i], z) with X = d_c (nj), Y = d_a (ni); d_z and d_s are not read */
#define CAF_LOCATE_TD 1       /* the e terms alone: velocities, d and wd are never read                             */
#define CAF_LOCATE_FD 2       /* the f terms alone                                                                  */
#define CAF_LOCATE_TDFD 3
typedef struct {
    int32_t source;         /* CAF_LOCATE_POINTS, CAF_LOCATE_MESH or CAF_LOCATE_MESH_XY                              */
    int32_t mode;           /* CAF_LOCATE_TD, CAF_LOCATE_FD or CAF_LOCATE_TDFD                                       */
    int32_t cost_f32;       /* 1: d_cost is float32 (the float64 cost rounded once), 0: float64                     */
    int32_t reserved;
    int64_t n;              /* CAF_LOCATE_POINTS: rows of d_points                                                   */
    const double* d_points;
    int32_t ni, nj;         /* the meshes: ni nj points                                                              */
    const double* d_a;      /* [ni] */
    const double* d_z;      /* [ni] */
    const double* d_c;      /* [nj] */
    const double* d_s;      /* [nj] */
    double z;               /* CAF_LOCATE_MESH_XY: the constant third coordinate                                     */
} caf_locate_desc;
/* d_records: K records of 16 doubles, s1(3) s2(3) v1(3) v2(3) r wr d wd.  d_set_starts (optional, DEVICE, B + 1 increasing
 * offsets from 0 to K) cuts the table into B sets of at least one record each: B cost grids over the same points in one
 * launch (offsets are clamped into [0, K], so no content of that array reaches outside the table); NULL: B = 1.
 * Outputs, each optional: d_cost (B, N) float64 or float32; d_min_val (B) float64 and d_min_idx (B) int64, the minimum of
 * each set's costs and the FIRST index that has it.  A NaN cost (an FD term at a point that coincides with a sensor is 0 / 0)
 * is stored as NaN and never wins; a set with nothing but NaN reports (NaN, -1). */
CAF_EXPORT int32_t caf_locate_grid(const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts,
                                   int32_t B, void* d_cost, double* d_min_val, int64_t* d_min_idx, void* stream);
/* the launch geometry: points per workgroup and records per staged chunk (the sizes at which the kernel changes path) */
CAF_EXPORT int32_t caf_locate_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk);
/* One-bounce round trips over the same grids (localizationRoutines.py:368-507: gridSearchRTT, gridSearchBlindLinearRTT), float64,
 * contraction off, no atomics.  Of the record, s1 is the transmitter, s2 the receiver, slot 12 the measured range sum r, slot 13
 * its weight w and slots 6 and 7 the nuisance basis g0, g1; the other slots are not read.  With d_k = r_k - (rho1_k + rho2_k):
 *   nuisance 0: cost[p] = sum_k w_k d_k^2, in the order of k;
 *   nuisance 1, 2: g0 (and g1) are orthonormal under the weights of their set, sum_k w g_i g_j = delta_ij; a first pass forms
 *     alpha = sum_k w g0 d (and beta = sum_k w g1 d), a second pass cost[p] = sum_k w (d - alpha g0 - beta g1)^2, which is
 *     min over (a, b) of sum_k w (d - a t - b)^2 for a basis of span{1} (and {1, t}).  Every range is computed twice.
 * desc (desc->mode is not read), d_records, K, d_set_starts (clamped), B and the three optional outputs are taken as
 * caf_locate_grid takes them; the first index wins the arg min, NaN never wins, nothing but NaN reports (NaN, -1).  A point on
 * a sensor has that range 0 and a finite cost.  Refused: nuisance outside 0..2, K < B (nuisance + 1), and what caf_locate_grid
 * refuses.  The offsets live on the device, so a SET with no more than `nuisance` records is NOT caught here (its cost is 0
 * everywhere): the caller refuses it, as it supplies the orthonormal basis. */
CAF_EXPORT int32_t caf_locate_rtt(const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts,
                                  int32_t B, int32_t nuisance, void* d_cost, double* d_min_val, int64_t* d_min_idx, void* stream);
CAF_EXPORT int32_t caf_locate_rtt_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk);

/* ---- CRB accuracy maps (crbRoutines.py: CRBMap).  Added after ABI 1.10 without a version bump, detected by symbol.  Everything
 * is float64.  The Cramer-Rao bound of a position fix at every point of the grids that caf_locate_grid searches: a record
 * (s1, s2, v1, v2, w, kind, 0, 0) adds w J J^T to the point's 3 x 3 Fisher matrix F, in the order of k, with a = p - s, rho = |a|,
 * u = a / rho.  The library knows nothing of seconds, hertz or radians: w is the weight of J in the units of J. */
#define CAF_CRB_RANGE 1       /* J = u1: a range from s1 (TOA)                                                     */
#define CAF_CRB_RANGE_SUM 2   /* J = u1 + u2: a one-bounce round trip, transmitter s1, receiver s2                 */
#define CAF_CRB_RANGE_DIFF 3  /* J = u2 - u1: a range difference (TDOA)                                            */
#define CAF_CRB_RATE_DIFF 4   /* J = g2 - g1, g = (v - u (u.v)) / rho: a range-rate difference of a stationary emitter,
                                 the gradient of the f term of the geolocation block above                         */
#define CAF_CRB_AOA3D 5       /* two rows about s1, azimuth and elevation, weights w cos^2(elevation) and w; NaN straight
                                 above or below the sensor                                                         */
#define CAF_CRB_FREE 0        /* CRB = F^-1                                                                        */
#define CAF_CRB_FIXED 1       /* the fix lies in the plane of normal n, `normal` for every point                   */
#define CAF_CRB_RADIAL 2      /* n = p (a known length of the position vector)                                     */
#define CAF_CRB_WGS84 3       /* n = (px / a^2, py / a^2, pz / b^2), the normal of the WGS84 ellipsoid through p   */
/* desc: source, n and the tables as for caf_locate_grid (desc->mode is not read; desc->cost_f32 chooses the type of d_rms);
 * d_records, K, d_set_starts, B as for caf_locate_grid: B maps over the same points in one launch.  A record of any other kind
 * makes every point of its set NaN.  A point on a sensor is NaN (0 / 0).  `normal`: HOST, 3 doubles, read for CAF_CRB_FIXED only.
 * Under a constraint, e = z^ x n (x^ where that vanishes), east = e / |e|, north = n^ x east, U = [east north],
 * G = U^T F U, C2 = G^-1 and CRB = U C2 U^T.  A point is unobservable, and NaN in every output, when a pivot of the L D L^T of G
 * (of F for CAF_CRB_FREE) is not above singular_threshold times its diagonal entry.
 * Outputs, each optional: d_crb (B, N, 6) = xx xy xz yy yz zz; d_ellipse (B, N, 3) = sigma_major >= sigma_minor (the roots of the
 * eigenvalues of C2) and the angle of the major axis from east toward north in (-pi/2, pi/2] (refused with CAF_CRB_FREE);
 * d_rms (B, N) float64 or float32 = sqrt(trace CRB); d_min_val / d_min_idx and d_max_val / d_max_idx (B): the extremes of each
 * set's rms and the FIRST index that has them (an index needs its value).  NaN never wins; nothing but NaN reports (NaN, -1). */
CAF_EXPORT int32_t caf_crb_map(const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts,
                               int32_t B, int32_t constraint, const double* normal, double* d_crb, double* d_ellipse, void* d_rms,
                               double* d_min_val, int64_t* d_min_idx, double* d_max_val, int64_t* d_max_idx, void* stream);
/* the launch geometry (points per workgroup, records per staged chunk) and the threshold of an unobservable point */
CAF_EXPORT int32_t caf_crb_map_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk, double* singular_threshold);

/* ---- Direct position determination (localizationRoutines.py: gridSearchCAF_direct, DPDMixin; caf_dpd.hip).  Added after ABI 1.10
 * without a version bump, detected by symbol.  CAF surfaces are added up over the grids that caf_locate_grid searches, with no
 * per-pair decision.  Record k = (s1, s2, v1, v2) (slots 0..11 of the 16 doubles; the rest are not read) comes with map k.  For a
 * grid point p, in float64 with k_locate's operations, contraction off:
 *   x = rho2 - rho1,  y = u2 - u1,  u_i = (p - s_i).v_i / rho_i,   a = (x - r0) inv_dr,  b = (y - d0) inv_dd.
 * The lookup is in range when 0 <= a <= nd - 1 and 0 <= b <= nf - 1 (a NaN coordinate is out of range).  In range:
 * i = min(floor(a), nd - 2), t = a - i, j and s from b in the same way, and with lerp(p, q, t) = fma(t, q - p, p)
 *   value = lerp(lerp(S[i, j], S[i, j + 1], s), lerp(S[i + 1, j], S[i + 1, j + 1], s), t),   S[i, j] = d_surface[i stride_d + j stride_f];
 * out of range: value = fill, and the record is no hit.  score[p] = sum_k w_k value_k, in the order of k, one fma per record.
 * A NaN among the four corners of the touched cell makes the score NaN.  The library knows nothing of seconds, hertz or carriers.
 * desc->grid.mode: CAF_LOCATE_TD maps have nf == 1 and nd >= 2 (velocities, d0 and inv_dd are never read, one lerp),
 * CAF_LOCATE_FD maps nd == 1 and nf >= 2, CAF_LOCATE_TDFD maps nd >= 2 and nf >= 2.  Every load lies inside [0, nd) x [0, nf) of
 * its map for every input; offsets are 64-bit, strides may be negative. */
typedef struct caf_dpd_map {
    const float* d_surface; /* DEVICE: the element (0, 0) of the map, float32                                            */
    int32_t nd, nf;         /* entries along a (range difference) and along b (range-rate difference)                   */
    int64_t stride_d;       /* in elements: rows of a (S, F) surface, of the (F, S) transpose and windows are all views */
    int64_t stride_f;
    double r0, inv_dr;      /* a = (x - r0) inv_dr                                                                      */
    double d0, inv_dd;      /* b = (y - d0) inv_dd                                                                      */
    double w;               /* the weight of the map in the score                                                       */
    double fill;            /* the value of a lookup out of range                                                       */
} caf_dpd_map;
/* grid: source, n and the tables as for caf_locate_grid; grid.cost_f32 chooses the type of d_score.  d_records, K, d_set_starts
 * (clamped), B as for caf_locate_grid: B score grids over the same points in one launch.  h_maps: HOST, K maps, checked before
 * anything touches a device (sizes for the mode; finite r0, inv_dr, d0, inv_dd, w, fill; no NULL surface; no zero stride of an
 * axis with more than one entry; K <= 2^20), then copied into a staging block the library keeps, uploaded into a pooled block on
 * desc->stream and given back to the pool when an event behind the launch has completed: the caller's array is free again on
 * return.  Outputs, each optional: d_score (B, N) float64, or float32 (the float64 score rounded once); d_hits (B, N) int32,
 * the records of the set that were in range; d_max_val (B) float64 and d_max_idx (B) int64, the maximum of each set's scores
 * and the FIRST index that has it.  NaN never wins; a set with nothing but NaN reports (NaN, -1).  No atomics: a set gives the
 * same bits alone and anywhere in a batch, for any choice of outputs, on every run.  All device work of the call is queued on
 * desc->stream and nowhere else, and the call does not wait for it. */
typedef struct caf_dpd_desc {
    caf_locate_desc grid;
    const double* d_records;     /* DEVICE (K, 16) */
    int64_t K;
    const int64_t* d_set_starts; /* DEVICE (B + 1), or NULL: B = 1 */
    int32_t B;
    int32_t reserved;
    const caf_dpd_map* h_maps;   /* HOST (K) */
    void* d_score;
    int32_t* d_hits;
    double* d_max_val;
    int64_t* d_max_idx;
    void* stream;
} caf_dpd_desc;
CAF_EXPORT int32_t caf_dpd_grid(const caf_dpd_desc* desc);
/* the launch geometry: points per workgroup and records per staged chunk (the sizes at which the kernel changes path) */
CAF_EXPORT int32_t caf_dpd_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk);

/* ---- CFAR detection on CAF surfaces (xcorrRoutines.py: cfarDetect; caf_cfar.hip).  Added after ABI 1.10 without a version bump,
 * detected by symbol.  For the cell (i, j) of a map, v = S[i, j] = d_surface[i stride_d + j stride_f], Hd = gd + td, Hf = gf + tf:
 *   ring: the cells (i + a, j + b) with |a| <= Hd and |b| <= Hf, not both |a| <= gd and |b| <= gf, 0 <= i + a < nd (the delay
 *     axis never wraps), the column in range (with wrap_f it is taken modulo nf, and 2 Hf + 1 <= nf is required), the value finite.
 *     R = the float64 sum of the ring in a fixed order, n = its size.
 *   noise: CAF_CFAR_CA: R / n, one float64 division (NaN for n = 0).  CAF_CFAR_GO / _SO: half A is the ring cells whose offset on
 *     split_axis is negative, half B those where it is positive (offset 0 is in neither); the larger (GO) or smaller (SO) of
 *     R_A / n_A and R_B / n_B over the halves that are not empty (NaN if both are), n = n_A + n_B.
 *   a detection: v finite, n >= min_cells, v >= floor, (double) v > alpha * noise (one product), and v the local maximum of its
 *     (2 md + 1) x (2 mf + 1) window under the same range and wrap rules: v > q for a neighbour q that precedes (i, j) in row-major
 *     (i, j) order, v >= q for one that follows, non-finite neighbours skipped -- a plateau gives its first cell exactly once.
 *   di: with p = S[i - 1, j], q = S[i + 1, j] as doubles: 0 if either is out of range or non-finite or den = (p - 2 v) + q >= 0,
 *     else (0.5 (p - q)) / den clamped to [-0.5, 0.5] and rounded to float32 once; dj alike along frequency, honouring wrap_f.
 *   noise = the float64 noise rounded once, ratio = (double) v / noise rounded once, cells = n.
 * Map b's detections go to d_det[b, 0 .. min(count, cap)) in row-major (i, j) order, d_count[b] is the full count, records past
 * the count are not written.  d_noise, where given, gets every cell's noise, NaN where n < min_cells.  No atomics: a map gives
 * the same bits alone and anywhere in a batch, for any choice of outputs, on every run. */
#define CAF_CFAR_CA 0
#define CAF_CFAR_GO 1
#define CAF_CFAR_SO 2
typedef struct caf_cfar_map {
    const float* d_surface; /* DEVICE: the element (0, 0) of the map, float32                                            */
    int32_t nd, nf;         /* delays and frequencies, each >= 1                                                        */
    int64_t stride_d;       /* in elements, not 0 on an axis with more than one entry, may be negative: (S, F) surfaces, */
    int64_t stride_f;       /* (F, S) rows of surface_t and windows of either are all views                             */
    double alpha, floor;    /* finite, alpha > 0                                                                        */
    float* d_noise;         /* DEVICE (nd, nf) compact row-major float32, or NULL                                       */
} caf_cfar_map;
typedef struct caf_cfar_det {
    int32_t i, j;
    float value, noise, ratio, di, dj;
    int32_t cells;
} caf_cfar_det; /* 32 bytes */
/* h_maps: HOST, B maps (1 <= B <= 2^20, sizes may differ), checked before anything touches a device, then staged, uploaded into a
 * pooled block on desc->stream and given back to the pool when an event behind the launches has completed: the caller's array is
 * free again on return.  Limits: gd, gf, td, tf >= 0; Hd, Hf <= 32; td + tf >= 1; 0 <= md <= Hd, 0 <= mf <= Hf, md + mf >= 1;
 * GO and SO need a half width >= 1 on split_axis; min_cells >= 0; cap >= 0, and d_det with a cap above 0; at most 2^31 - 1 tiles
 * of 32 x 32 cells per call.  d_count may be NULL.  All device work of the call is queued on desc->stream and nowhere else; the
 * call waits for nothing and reads no count back. */
typedef struct caf_cfar_desc {
    const caf_cfar_map* h_maps; /* HOST (B) */
    int32_t B;
    int32_t gd, gf, td, tf;     /* guard and training half widths */
    int32_t md, mf;             /* half widths of the local-maximum window */
    int32_t mode;               /* CAF_CFAR_CA, _GO, _SO */
    int32_t split_axis;         /* 0 = delay, 1 = frequency; read for GO and SO */
    int32_t wrap_f, min_cells;
    caf_cfar_det* d_det;        /* DEVICE (B, cap) */
    int64_t cap;
    int64_t* d_count;           /* DEVICE (B): the true count, also beyond cap */
    void* stream;
} caf_cfar_desc;
CAF_EXPORT int32_t caf_cfar_surface(const caf_cfar_desc* desc);
/* the launch geometry at half widths (Hd, Hf): the cells of a tile on each axis (the sizes at which the kernel changes path), the
 * threads of a workgroup and the most LDS it takes, in bytes (GO / SO split on frequency; CA and a split on delay take less) */
CAF_EXPORT int32_t caf_cfar_geometry(int32_t Hd, int32_t Hf, int32_t* tile_d, int32_t* tile_f, int32_t* threads, int64_t* lds_bytes);

/* ---- Lines of position on an oblate spheroid (hyperboloidRoutines.py: Hyperboloid.intersectOblateSpheroid; sphereRoutines.py:
 * Sphere.intersectOblateSpheroid).  Added after ABI 1.10 without a version bump, detected by symbol.  Everything is float64,
 * contraction off, no atomics.  A job is 16 doubles, mu(3) e0(3) e1(3) e2(3) a c p_min p_max, and describes the family of circles
 *   q(phi) = C(p) + A(p) cos phi + B(p) sin phi,
 *   CAF_LOP_HYPERBOLOID: C = mu - c cosh p e2, A = a sinh p e0, B = a sinh p e1   (the sheet of range difference 2 c, p = v >= 0)
 *   CAF_LOP_SPHERE:      C = mu + c cos p e2,  A = a sin p e0,  B = a sin p e1    (a = c = r, p = theta in [0, pi])
 * cut with E(q) = (qx^2 + qy^2) / omega^2 + qz^2 / lambda^2 - 1 = 0.  With C^ = (Cx / omega, Cy / omega, Cz / lambda) (A^, B^ alike),
 *   g(phi) = E(q(phi)) = k0 + k1 cos phi + k2 sin phi + k3 cos 2 phi + k4 sin 2 phi,
 *   k0 = C^.C^ + (A^.A^ + B^.B^) / 2 - 1, k1 = 2 C^.A^, k2 = 2 C^.B^, k3 = (A^.A^ - B^.B^) / 2, k4 = A^.B^,
 * which has at most four zeros in (-pi, pi].  A job with A = B = 0 at p, or with anything that is not finite, has no zero at p.
 * Every loop of both kernels has a trip count fixed at compile time. */
#define CAF_LOP_HYPERBOLOID 0
#define CAF_LOP_SPHERE 1
#define CAF_LOP_LIST 0        /* sample j of every job takes d_p[j]                                                      */
#define CAF_LOP_LINSPACE 1    /* lo + j ((hi - lo) / (P - 1)); the last sample is hi itself; P = 1: lo                    */
#define CAF_LOP_CHEBYSHEV 2   /* lo + (hi - lo) (1 - cos(pi (j + 1/2) / P)) / 2: dense towards both ends                  */
#define CAF_LOP_FOUND 0       /* d_status of caf_lop_range: some parameter of the search has a zero                       */
#define CAF_LOP_NO_CURVE 1    /* none has: the range is (NaN, NaN)                                                        */
typedef struct {
    int32_t kind;           /* CAF_LOP_HYPERBOLOID or CAF_LOP_SPHERE                                                  */
    int32_t spacing;        /* CAF_LOP_LIST, CAF_LOP_LINSPACE or CAF_LOP_CHEBYSHEV (caf_lop_range does not read it)   */
    int32_t P;              /* samples per job (caf_lop_range does not read it)                                       */
    int32_t reserved;
    double omega, lambda;   /* the semi-axes of the spheroid: x and y, and z                                          */
    const double* d_p;      /* CAF_LOP_LIST: [P], shared by every job                                                 */
} caf_lop_desc;
/* d_jobs (B, 16).  d_range (B, 2) = (lo, hi) of each job, read for CAF_LOP_LINSPACE and CAF_LOP_CHEBYSHEV.  Outputs, each optional,
 * one entry per (job, sample): d_count (B, P) int32, the number of zeros, 0..4; d_phi (B, P, 4), the zeros ascending in
 * (-pi, pi], then NaN; d_xyz (B, P, 4, 3) = q(phi); d_latlon (B, P, 4, 2), geodetic degrees of a point of the surface,
 * latitude = atan2(z / lambda^2, hypot(x, y) / omega^2), longitude = atan2(y, x); d_p_out (B, P), the parameter of the sample.
 * One thread per (job, sample).  Refused: NULL desc or jobs, unknown kind or spacing, semi-axes not finite and positive, B < 1,
 * P < 1, B P beyond one launch, CAF_LOP_LIST without d_p, the other spacings without d_range. */
CAF_EXPORT int32_t caf_lop_points(const caf_lop_desc* desc, const double* d_jobs, int64_t B, const double* d_range, int32_t* d_count,
                                  double* d_phi, double* d_xyz, double* d_latlon, double* d_p_out, void* stream);
/* The interval of [p_min, p_max] of each job on which g has a zero, one wave per job: round 0 tries `width` parameters
 * p_min + i (p_max - p_min) / (width - 1); every later round tries `width` parameters strictly inside the bracket (a, b) between the
 * first (last) parameter with a zero and its neighbour without, a + (i + 1) (b - a) / (width + 1).  d_range (B, 2): the smallest and
 * the largest parameter found to have a zero, each a parameter at which caf_lop_points finds one too (the same device function);
 * d_status (B) int32.  Both optional.  Refused: as above, without P, spacing and d_p. */
CAF_EXPORT int32_t caf_lop_range(const caf_lop_desc* desc, const double* d_jobs, int64_t B, double* d_range, int32_t* d_status,
                                 void* stream);
/* samples per workgroup of caf_lop_points, jobs per workgroup of caf_lop_range, and the number and width of its search rounds */
CAF_EXPORT int32_t caf_lop_geometry(int32_t* samples_per_workgroup, int32_t* jobs_per_workgroup, int32_t* rounds, int32_t* width);

/* ---- Viterbi sequence detection (viterbiDemodClasses.py: ViterbiDemodulator, BurstyViterbiDemodulator).  Added after ABI 1.10
 * without a version bump, detected by symbol.  Everything is float64.  With A states, T pretransitions per state, L sources:
 *   P_n[m] = sum_i exp(-j omegas[i] (n up + m)) pulses[i][m], m < pulselen, and the signal of a symbol sequence g is
 *   x[w] = sum_k g[k] P_k[w - k up].  Step n of state p over its pretransitions q: long = |y - x|^2 over [n up, n up + pulselen)
 *   with the survivor of q followed by alphabet[p], short = the same over the first up samples; the FIRST minimum of the long
 *   metric alone wins, and the path metric grows by the winner's short metric.  (csrc/caf_viterbi.hip has the whole rule.) */
/* d_table (pathlen, pulselen) complex128 = P_n[m] from d_pulses (L, pulselen) complex128 and d_omegas (L) float64 */
CAF_EXPORT int32_t caf_viterbi_table(const double* d_pulses, const double* d_omegas, int32_t L, int32_t pulselen, int32_t up,
                                     int32_t pathlen, double* d_table, void* stream);
typedef struct {
    int32_t num_states;             /* A, 1..8                                                                          */
    int32_t num_trans;              /* T, 1..A                                                                          */
    int32_t up;                     /* samples per symbol, >= 1                                                         */
    int32_t pulselen;               /* up..512                                                                          */
    int32_t pathlen;                /* symbols per row, >= 1                                                            */
    int32_t num_burst_syms;         /* 0 (with num_guard_syms = 0): no burst period, the plain class                    */
    int32_t num_guard_syms;         /* a new-burst step every num_burst_syms + num_guard_syms symbols                   */
    int32_t y_c128;                 /* 1: d_y is complex128, 0: complex64                                               */
    const double* h_alphabet;       /* HOST: A complex128 values                                                        */
    const int32_t* h_pretransitions;/* HOST: (A, T), every entry in [0, A)                                              */
    const int32_t* h_allowed;       /* HOST: the states that may start (a burst), num_allowed of them in [0, A)         */
    int32_t num_allowed;
    int32_t reserved;
    const double* d_table;          /* caf_viterbi_table of the same pulselen and up, at least pathlen rows             */
    const void* d_y;                /* (rows, ylength), ylength >= (pathlen - 1) up + pulselen                          */
    int64_t rows, ylength;
    uint8_t* d_states;              /* outputs, each optional: (rows, A, pathlen) state per slot, 255 = never written   */
    double* d_metrics;              /* (rows, A) path metrics, +inf for a state without a survivor                      */
    int32_t* d_best;                /* (rows) the first arg min of the path metrics                                     */
    uint8_t* d_best_path;           /* (rows, pathlen) = d_states[row][best]                                            */
} caf_viterbi_desc;
/* Every row of either class in one launch; rows are independent and a row's outputs do not depend on the batch.  What is not
 * supported (more than 8 states, pulselen > 512, a short row, a pretransition outside [0, A)) is refused with CAF_ERR_INVALID
 * before anything is launched; there is no other path. */
CAF_EXPORT int32_t caf_viterbi_demod(const caf_viterbi_desc* desc, void* stream);
/* the limits and the traceback chunk (the size at which the kernel changes path) */
CAF_EXPORT int32_t caf_viterbi_geometry(int32_t* max_states, int32_t* max_pulselen, int32_t* decision_chunk);

/* ---- Signal propagation and tones (signalCreationRoutines.py: propagateSignal :296-328, propagateSignalExact :331-353,
 * freqshiftSignal :398-418, cupyAddTonePhase :454-487, cupyGenTonesDirect / cupyGenTonesScaling :500-560).  Added after ABI 1.10
 * without a version bump, detected by symbol.  Signals and results are complex64; every phase is formed and reduced to a
 * fraction of a turn in float64 (csrc/caf_propagate.hip).  k' is the signed bin of makeFreq: k for 2 k < len, k - len otherwise,
 * so for even len bin len / 2 is -fs / 2. */
/* propagateSignal: d_out (num_delays, len) = IFFT( FFT(d_sig row r, or the one row when rows_sig == 1) exp(-j 2 pi f_k t_r) ),
 * f_k = k' fs / len, d_time (num_delays) float64 seconds, times d_tone (len complex64) when that is not NULL.  Any len. */
CAF_EXPORT int32_t caf_propagate(const float* d_sig, int32_t rows_sig, int64_t len, const double* d_time, int32_t num_delays,
                                 double fs, const float* d_tone, float* d_out, void* stream);
/* propagateSignalExact for one signal row d_sig (len) and `rows` rows of delays d_tau (rows, len) float64 seconds:
 * d_out[r][n] = exp(-j 2 pi f_c tau[r][n]) (1 / len) sum_k X[k] exp(j 2 pi (n / fs - tau[r][n]) f_k), X = FFT(d_sig).
 * len^2 terms per row; 1 <= len <= 2^20, anything else is refused with CAF_ERR_INVALID before a launch.  Deterministic, and a
 * row's result does not depend on the other rows. */
CAF_EXPORT int32_t caf_propagate_exact(const float* d_sig, const double* d_tau, int32_t rows, int32_t len, double fs, double f_c,
                                       float* d_out, void* stream);
/* the limits and tile sizes of caf_propagate_exact (the sizes at which the kernel changes path, and the rotor's re-seed
 * interval, on which its error bound depends) */
CAF_EXPORT int32_t caf_propagate_geometry(int32_t* max_len, int32_t* reseed_interval, int32_t* outputs_per_workgroup,
                                          int32_t* waves_per_workgroup);
/* genTones{Direct,Scaling}_{64f,32f}: d_out (num_freqs, length) complex128 (c128 = 1) or complex64, row i =
 * exp(j pi (2 (f0 + i fstep) n)), the phase in float64.  Every row is computed directly: the Scaling kernels' accumulated
 * drift is not reproduced. */
CAF_EXPORT int32_t caf_gen_tones(double f0, double fstep, int32_t num_freqs, int64_t length, int32_t c128, void* d_out,
                                 void* stream);
/* addPhase, in place: d_phase[i] = (float)fma(2 pi freq, fma(i, tstep, tstart), d_phase[i]), the arithmetic in float64 */
CAF_EXPORT int32_t caf_add_tone_phase(float* d_phase, int64_t len, double freq, double tstart, double tstep, void* stream);
/* d_out[r][i] = d_x[r][i] exp(j 2 pi fnorm i), fnorm in cycles per sample (freqshiftSignal with fnorm = freq / fs) */
CAF_EXPORT int32_t caf_freq_shift(const float* d_x, int64_t rows, int64_t len, double fnorm, float* d_out, void* stream);

/* ---- Subspace spectra (musicRoutines.py: MUSIC, CAPON, ESPRIT, musicAlg; xcorrRoutines.py: musicXcorr :378-410).  Added after
 * ABI 1.10 without a version bump, detected by symbol.  All arithmetic is float64, nothing is atomic, and entry b of a batch is
 * bitwise what the same problem gives alone (csrc/caf_music.hip).  Matrices are row-major complex128 (re, im pairs). */
/* the limits: rows of a covariance, the sweep limit of the eigensolver, the covariance tile (the size at which the kernel takes
 * another workgroup) and the largest batch of one call */
CAF_EXPORT int32_t caf_music_geometry(int32_t* min_rows, int32_t* max_rows, int32_t* max_sweeps, int32_t* cov_tile, int32_t* max_batch);
/* Snapshot covariances: d_rx (batch, rows, rows), Rx[i][j] = h_scale[b] sum_segments sum_c x[c jump + i] conj(x[c jump + j]).
 * d_x: x_len elements, complex128 (x_c128 = 1) or complex64.  h_segs: (batch, nseg, 3) int64 (offset, element stride, length) in
 * elements of d_x; a segment gives (length - rows) / jump + 1 snapshots (snapshotJump = None of the reference is jump = rows) and
 * must lie inside d_x with length >= rows.  fwd_bwd: 0.5 (Rx + J Rx^T J); toeplitz: every diagonal replaced by its mean, after
 * that. */
CAF_EXPORT int32_t caf_music_cov(const void* d_x, int32_t x_c128, int64_t x_len, const int64_t* h_segs, int32_t nseg, int32_t batch,
                                 int32_t rows, int64_t jump, const double* h_scale, int32_t fwd_bwd, int32_t toeplitz, double* d_rx,
                                 void* stream);
/* Hermitian eigendecompositions of d_rx (batch, rows, rows) by one-sided Jacobi: d_s (batch, rows) descending, d_u (batch, rows,
 * rows) the unit eigenvectors as columns in that order (the phase of a column is unspecified), d_vh = u^H (or NULL).
 * d_status (batch) int32: the sweeps used, or -1 where the sweep limit ran out (the outputs of that entry are then not to be
 * used; the call itself still returns CAF_OK). */
CAF_EXPORT int32_t caf_music_eig(const double* d_rx, int32_t batch, int32_t rows, double* d_s, double* d_u, double* d_vh,
                                 int32_t* d_status, void* stream);
/* Pseudo-spectra: with g_k(f) = |sum_m exp(-j 2 pi f m) u[m][k]|^2, denom_p = sum_{k >= p} g_k and num_p = sum_{k < p} g_k / s_k:
 * mode 0: d_f = 1 / denom_p; mode 1: num_p / denom_p (the signal subspace as numerator); mode 2 (Capon, np = 1, h_plist ignored):
 * 1 / sum_k g_k / s_k.  d_freqs (nfreq) float64 cycles per sample; h_plist (np) int32, 0 <= p < rows; d_f (batch, np, nfreq)
 * float64; d_denom / d_num: the same shape, or NULL. */
CAF_EXPORT int32_t caf_music_spectrum(const double* d_u, const double* d_s, int32_t batch, int32_t rows, const double* d_freqs,
                                      int32_t nfreq, const int32_t* h_plist, int32_t np, int32_t mode, double* d_f, double* d_denom,
                                      double* d_num, void* stream);
/* The filtered products of musicXcorr: d_out (batch, len) complex128, row b = lfilter(taps, 1, rx[s_b : s_b + len] conj(cutout)),
 * direct form.  d_rx (rx_len), d_cutout (len), d_taps (ntaps) complex128; h_shifts (batch) int64, 0 <= s_b <= rx_len - len. */
CAF_EXPORT int32_t caf_music_xcorr_front(const double* d_rx, int64_t rx_len, const double* d_cutout, int64_t len, const double* d_taps,
                                         int32_t ntaps, const int64_t* h_shifts, int32_t batch, double* d_out, void* stream);

/* ---- Moving-platform scenarios (trajectoryRoutines.py: Trajectory.to / frm; cython_ext/PySampledLinearInterpolator: the
 * ConstAmpSigLerp family).  Added after ABI 1.10 without a version bump, detected by symbol.  All arithmetic is float64, nothing
 * is atomic, one thread per (row, sample): a row is bitwise the same whatever the number of rows (csrc/caf_scene.hip).
 * The small tables are host arrays (h_), read and checked before a launch; the long ones are device arrays (d_). */
#define CAF_TRAJ_STATIONARY 0
#define CAF_TRAJ_CONSTANT_VELOCITY 1
#define CAF_TRAJ_INTERPOLATED 2
typedef struct caf_traj_table {
    int32_t count;             /* trajectories */
    int32_t reserved;
    const int32_t* h_kind;     /* (count) CAF_TRAJ_* */
    const double* h_x0v;       /* (count, 6) x0 and v, metres and metres per second; z = 0 for a 2-D trajectory.  An interpolated
                                * trajectory's row is not read. */
    const int64_t* h_knot_off; /* (count + 1) trajectory i owns knots h_knot_off[i] .. h_knot_off[i + 1] of d_tp / d_xp: at least
                                * 2 for an interpolated one, none otherwise */
    const double* d_tp;        /* (h_knot_off[count]) knot times, strictly increasing within a trajectory; NULL without knots */
    const double* d_xp;        /* (h_knot_off[count], 3) knot positions; piecewise linear, held at the end knots outside tp */
} caf_traj_table;
typedef struct caf_burst_table {
    int32_t count;              /* emitters (signals) */
    int32_t reserved;
    const int32_t* h_burst_off; /* (count + 1) emitter e owns bursts h_burst_off[e] .. h_burst_off[e + 1], at least one */
    const double* h_burst;      /* (bursts, 7): timevec[0], timevec[-1] - timevec[0], T, amp, fc, phi, tJump.  Within an emitter
                                 * the emission windows are in ascending order and disjoint as float64 computes them:
                                 * (timevec[0] + tJump) + span of a burst <= timevec[0] + tJump of the next. */
    const int64_t* h_phase_off; /* (bursts + 1) burst b owns d_phase[h_phase_off[b] .. h_phase_off[b + 1]], at least 2 knots, and
                                 * span <= (knots - 1 + 1e-3) T (the last segment serves what lies past the last knot) */
    const double* d_phase;      /* the phase tables, radians, knot k at timevec[0] + k T */
} caf_burst_table;
/* the limits: emitters, receivers (rows of caf_traj_tau and of caf_scene_propagate), bursts per emitter, knots of all trajectories
 * of a table together, and the threads (= outputs) per workgroup */
CAF_EXPORT int32_t caf_scene_geometry(int32_t* max_emitters, int32_t* max_receivers, int32_t* max_bursts, int64_t* max_knots,
                                      int32_t* threads_per_workgroup, int32_t* outputs_per_workgroup);
/* Light times.  d_tau (others->count, n) float64: row r is self.to(other_r, d_t) (direction 0: the photon leaves self at t) or
 * self.frm(other_r, d_t) (direction 1: it arrives at self at t), the solution of c tau = |p_self(t) - p_other(t +- tau)|.
 * self holds one trajectory.  A stationary other: distance / c.  A constant-velocity other with method 0 and a self that is
 * not interpolated: the quadratic in closed form.  Anything else (method 1, an interpolated side): 5 fixed-point steps from 0.
 * A constant-velocity speed of 1e-4 c or more is refused; the segments of an interpolated trajectory must be slower than that too
 * (not checked here: the knots are on the device), or the 5 steps do not reach float64. */
CAF_EXPORT int32_t caf_traj_tau(const caf_traj_table* self, const caf_traj_table* others, const double* d_t, int64_t n,
                                int32_t direction, int32_t method, double* d_tau, void* stream);
/* d_out[n] = sum_e sum_b amp exp(j (lerp(phase_b)(u) - 2 pi fc (tau[n] + tJump) + phi)), u = t[n] - tau[n] - tJump - timevec[0],
 * a term present iff 0 <= u < span; n < start_idx gives 0.  d_t, d_tau (n) float64; d_out (n) complex128 (c128 = 1) or
 * complex64.  The emitters are summed in order in float64 and rounded once. */
CAF_EXPORT int32_t caf_lerp_propagate(const caf_burst_table* bursts, const double* d_t, const double* d_tau, int64_t n,
                                      int64_t start_idx, int32_t c128, void* d_out, void* stream);
/* The same sum with t[n] = t0 + n dt and, for emitter e and receiver r, tau = receivers[r].frm(emitters[e], t[n]) solved in the
 * kernel (method 0): d_out (receivers->count, n).  emitters->count == bursts->count.  dt > 0.
 * Precondition, not checked here for knot tables (they are on the device): every segment of an interpolated emitter or receiver
 * is slower than 1e-4 c, and dt is many ulps of t0 + n dt, so that the emission time t - tau increases with n.  A workgroup
 * brackets the bursts of its first and last sample and looks no further; where the precondition fails, terms can be missing from
 * the result (no access leaves the tables).  The Python layer checks the speeds. */
CAF_EXPORT int32_t caf_scene_propagate(const caf_traj_table* emitters, const caf_traj_table* receivers, const caf_burst_table* bursts,
                                       double t0, double dt, int64_t n, int32_t c128, void* d_out, void* stream);

/* ---- Signal cancellation (cancellationRoutines.py: cancelSignalAtIdx :11-41, and the search over acceleration factors its
 * __main__ names).  Added after ABI 1.10 without a version bump, detected by symbol (csrc/caf_cancel.hip).  For job b with the
 * template s = d_sigs[b] (n_len complex64 samples), the start d_idx[b], a frequency nu (cycles per sample) and a rate alpha
 * (cycles per sample^2):
 *   m[n] = s[n] exp(+j 2 pi (nu n + alpha n^2 / 2)),  D = sum_n conj(m[n]) rx[idx + n],  Es = sum |s|^2,  Er = sum |rx[idx + n]|^2,
 *   amp = D / Es,  QF^2 = |D|^2 / (Es Er),  resid = Er - |D|^2 / Es,  cancelled[idx + n] = rx[idx + n] - amp m[n].
 * Phases are formed and reduced to a fraction of a turn in float64, products and rotors are float32, sums float64 in a fixed
 * order: nothing is atomic, and a job's outputs are bitwise the same alone and in a batch.  A window that does not lie wholly
 * inside rx (d_idx[b] < 0 or d_idx[b] + n_len > rx_len) is CAF_ERR_INVALID: the B indices are downloaded and checked before a
 * launch, so every call below blocks until earlier work on `stream` that wrote d_idx has finished. */
/* the limits (n_len, jobs, rates, frequencies of one call) and the sizes on which the error bound and the paths of the search
 * depend: template samples per work item, samples per thread, rotor steps between two float64 seeds */
CAF_EXPORT int32_t caf_cancel_geometry(int32_t* max_len, int32_t* chunk, int32_t* samples_per_thread, int32_t* reseed_interval,
                                       int32_t* max_jobs, int32_t* max_rates, int32_t* max_freqs);
/* D at the J rates d_rates[j] x the K frequencies nu0 + k dnu, for every job against the same d_rx, and the arg max of |D|^2
 * over (j, k) (the lower flat index j K + k wins ties).  Outputs, each (B) unless noted and each optional (NULL): d_best_j,
 * d_best_k int32; d_nu = nu0 + k dnu and d_rate = d_rates[j] of the winner; d_amp (B, 2) re, im; d_qf2, d_es, d_er, d_resid at
 * the winner; d_surface (B, J, K) float32 QF^2. */
CAF_EXPORT int32_t caf_cancel_search(const float* d_sigs, int32_t B, int32_t n_len, const float* d_rx, int64_t rx_len,
                                     const int32_t* d_idx, double nu0, double dnu, int32_t K, const double* d_rates, int32_t J,
                                     int32_t* d_best_j, int32_t* d_best_k, double* d_nu, double* d_rate, double* d_amp, double* d_qf2,
                                     double* d_es, double* d_er, double* d_resid, float* d_surface, void* stream);
/* the same estimate at one hypothesis per job: d_nu[b], d_rate[b] (the search's kernels with J = K = 1) */
CAF_EXPORT int32_t caf_cancel_estimate(const float* d_sigs, int32_t B, int32_t n_len, const float* d_rx, int64_t rx_len,
                                       const int32_t* d_idx, const double* d_nu, const double* d_rate, double* d_amp, double* d_qf2,
                                       double* d_es, double* d_er, double* d_resid, void* stream);
/* d_out[m] = d_rx[m] - sum_b d_amp[b] m_b[m - d_idx[b]] over the jobs whose window covers m, in increasing b, one float32
 * complex multiply-add each; other samples are copied.  d_out (rx_len) may be d_rx. */
CAF_EXPORT int32_t caf_cancel_subtract(const float* d_sigs, int32_t B, int32_t n_len, const float* d_rx, int64_t rx_len,
                                       const int32_t* d_idx, const double* d_nu, const double* d_rate, const double* d_amp,
                                       float* d_out, void* stream);

/* ---- The matrix profile of one record (matrixProfileRoutines.py: MatrixProfile, CupyMatrixProfile).  Added after ABI 1.10
 * without a version bump, detected by symbol (csrc/caf_mprofile.hip).  d_x holds n complex64 samples, 2 <= n < 2^31; for the
 * window w (1 <= w <= max_window, w < n) there are M = n - w + 1 window positions, and diagonal k (1 <= k <= M - 1) holds the
 * M - k values
 *   v(i, k) = |sum_{t < w} x[i + t] conj(x[i + k + t])|^2 / (E[i] E[i + k]),  E[i] = sum_{t < w} |x[i + t]|^2,  0 <= i < M - k.
 * Products, their running prefix, the energies and the quotient are float64 in a fixed order, the value is rounded once to
 * float32; a value is NaN where one of its two energies is zero.  Every call below computes the same bits for the same
 * (x, w, i, k), whatever diagonals it is asked for, and repeats them on every run.  Anything outside the limits is
 * CAF_ERR_INVALID; nothing is clamped. */
/* segment: window positions per work item; chunk: diagonals per work item; max_window: the longest w.  With n, w (and the
 * number of diagonals of a chains call) also the sizes that follow from them, 0 where n or w is out of range:
 * products_per_thread (the run of products a thread adds up before the workgroup's scan), the bytes of pooled scratch a
 * call takes (energies; energies + run counts + offsets of a chains call; energies + keys of a profile call) and the bytes
 * of LDS of a work item.  Every output is optional (NULL). */
CAF_EXPORT int32_t caf_mp_geometry(int64_t n, int32_t w, int64_t num_diagonals, int32_t* segment, int32_t* chunk,
                                   int32_t* max_window, int32_t* products_per_thread, int64_t* energy_bytes,
                                   int64_t* chains_bytes, int64_t* profile_bytes, int64_t* lds_bytes);
/* The diagonals k0 <= k < k1 (1 <= k0 < k1 <= M), packed one after the other: value (i, k) at
 * d_out[(k - k0) M - (k0 + k - 1) (k - k0) / 2 + i], an int64 offset; sum_{k0 <= k < k1} (M - k) floats in all. */
CAF_EXPORT int32_t caf_mp_raw(const float* d_x, int64_t n, int32_t w, int32_t k0, int32_t k1, float* d_out, void* stream);
/* The runs of v > min_threshold (compared as float32; NaN is never above) on the diagonals k0 <= k < k1, or, with d_diagonals
 * != NULL, on its num_diagonals diagonals (int32, strictly increasing, each within 1 .. M - 1; k0 and k1 are then not read;
 * the list is downloaded and checked first, so the call blocks until earlier work on `stream` that wrote it has finished).
 * A run is (k, start, end), end exclusive, cut at the multiples of `segment`: runs that meet there (the same k, one's end
 * the other's start) are one chain, and joining them is left to the caller.  *h_total (host memory) receives the number of
 * runs, complete on return; the first min(*h_total, capacity) runs in (k, start) order are written to d_runs (capacity, 3)
 * int32.  capacity == 0 counts only (d_runs may be NULL).  The list is the same on every run. */
CAF_EXPORT int32_t caf_mp_chains(const float* d_x, int64_t n, int32_t w, int32_t k0, int32_t k1, const int32_t* d_diagonals,
                                 int32_t num_diagonals, float min_threshold, int64_t capacity, int32_t* d_runs, int64_t* h_total,
                                 void* stream);
/* For every window position p < M the largest v over its partners q = p - k and q = p + k, kmin <= k <= kmax, 0 <= q < M
 * (1 <= kmin, kmax <= M - 1; kmin > kmax is an empty range): d_value (M) float32 and d_index (M) int32 = q.  Of equal values
 * the smallest k wins, and of equal k the left partner q = p - k.  NaN is never chosen; a position with no partner in range,
 * or with NaN for every partner, gets value 0 and index -1.  No diagonal is written anywhere. */
CAF_EXPORT int32_t caf_mp_profile(const float* d_x, int64_t n, int32_t w, int32_t kmin, int32_t kmax, float* d_value,
                                  int32_t* d_index, void* stream);

/* ---- cyclic-moment line search for batches of bursts (cyclostationaryRoutines.py: PSKOrderDetector, estimateOffsetViaCM,
 *      estimateBaud; caf_cyclo.hip) -------------------------------------------------------------------------------------
 * d_x: (rows, pitch) complex64.  d_lengths: int32 per row, or NULL (every row has `pitch` samples); row r uses its first
 * L_r <= min(pitch, nfft) samples and the transform is zero-padded to nfft.  moments / band_lo / band_hi are HOST arrays of
 * num_moments (1 .. 5) entries.  moments[k] selects the sequence that is transformed:
 *   0: z = |x| - mean(|x|)     1: z = |x|^2 - mean(|x|^2)     2, 4, 8: z = x^m by repeated complex squaring,
 * the mean over the row's own L_r samples (float64, in a fixed order), so that zero-padding does not spread a DC term.
 * The band of moment k is the signed bins band_lo[k] .. band_hi[k], inclusive, -nfft/2 <= lo <= hi <= (nfft - 1)/2, i.e. the
 * FFT-order indices b mod nfft.  Per (row, moment), at [row * num_moments + k]:
 *   d_index (int32)       FFT-order index of the largest |Z|^2 in the band, the lower index of equal values
 *   d_peak  (float64)     |Z[index]|
 *   d_side  (2 float64)   |Z[index - 1]|, |Z[index + 1]|, circular, in the band or not
 *   d_power (float64)     sum of |Z|^2 over the band
 * d_peak, d_side and d_power may be NULL.  A row of L_r = 0, a row of zeros and a sequence z of zeros give index -1 and zeros.
 * Every row is scaled by an exact power of two before it is raised (x^8 stays inside float32 at any level) and the outputs are
 * scaled back in float64.  A non-finite sample makes its own row's results unspecified and nothing else.  A row's results are
 * the same bits alone, in any batch and at any place in it.
 * nfft a power of two within 64 .. 16384: one launch, the spectra never leave the LDS; no scratch, asynchronous on `stream`
 * unless d_lengths is given (it is downloaded and checked first).  Any other nfft: elementwise kernel, rocFFT rows and a line
 * kernel per moment over pooled scratch.  CAF_CYCLO_DEBUG=1 names the form on stderr (`cm_lds nfft=... rows/wg=...` or
 * `cm_rocfft nfft=...`). */
CAF_EXPORT int32_t caf_cm_lines(const float* d_x, int64_t rows, int64_t pitch, const int32_t* d_lengths, int64_t nfft,
                                const int32_t* moments, int32_t num_moments, const int32_t* band_lo, const int32_t* band_hi,
                                int32_t* d_index, double* d_peak, double* d_side, double* d_power, void* stream);
/* form: 1 the in-LDS kernel, 2 the composed form, 0 nfft out of range; threads per workgroup, rows per workgroup and the
 * bytes of dynamic LDS of a workgroup.  Every output is optional (NULL).  No device work. */
CAF_EXPORT int32_t caf_cm_geometry(int64_t nfft, int32_t* form, int32_t* threads, int32_t* rows_per_wg, int64_t* lds_bytes);

/* ---- FAM spectral-correlation estimator (cyclostationaryRoutines.py: scfFAM, cycleLines, estimateBaudSCF; caf_scf.hip) ----
 * Per row x of n complex64 samples, a window a(n), n < N' = num_channels, a hop of L = hop samples, P = num_hops hops and a
 * smoothing g(r) >= 0, r < P (d_smooth == NULL: all ones), with signed channels k, l in [-N'/2, N'/2):
 *   X(k, r)    = sum_{n < N'} a(n) x(rL + n) e^{-j 2 pi k (rL + n) / N'}        (absolute phase, formed from (k (rL + n)) mod N')
 *   S(k, l, q) = sum_r g(r) X(k, r) conj(X(l, r)) e^{-j 2 pi q r / P}           (conjugate = 1 drops the conj)
 *   psd(k)     = sum_r g(r) |X(k, r)|^2                                          (float64)
 * M = P L / N' and q in [-M/2, M/2) is kept.  d = k - l, s = k + l, dmin = -(N' - 1) (conjugate form: d = k + l, s = k - l,
 * dmin = -N'); the cell (k, l, q) lies at cycle frequency alpha = (d M + q) fs / (P L) and frequency f = s fs / (2 N'), in
 * alpha-bin a = (d - dmin) M + (q + M/2) of A = (2 N' - 1) M.  A cell's value is |S|^2, or with coherence = 1
 * |S|^2 / (psd(k) psd(l)) (0 where the denominator is 0), formed in float64 from the float32 transform and rounded once to float32.
 *   d_scf        (rows, N', N', M) float32 at [k + N'/2][l + N'/2][q + M/2]
 *   d_alpha_val  (rows, A) float32: per alpha-bin the largest value over the pairs of its d
 *   d_alpha_arg  (rows, A) int32: the s of that pair, the smaller s of equal values
 *   d_psd        (rows, N') float64 at [k + N'/2]
 * Each output is optional (NULL); at least one is required.  Accepted: N' a power of two in 64 .. 1024, L a power of two in
 * 1 .. N'/4, P a power of two in 64 .. 16384, M >= 2, n >= (P - 1) L + N' (samples beyond that are not read), rows >= 1,
 * pitch >= n.  Everything else is CAF_ERR_INVALID before anything touches a device; there is no composed form.
 * Every output is the same bits alone, in any batch, at any place in it and on every run.  A non-finite sample spoils its own
 * row only (its values come out NaN or unspecified).  Pooled scratch of caf_scf_geometry's scratch_bytes_per_row per row, at
 * most 256 MiB of demodulates at a time.  CAF_SCF_DEBUG=1 prints one line per call on stderr (`[caf scf] fam np=... out=...`).
 * The stream is a field of the descriptor: all device work of the call is queued on desc->stream and nowhere else, as for every
 * entry point that ends in `void* stream`; tests/test_gpu_scf.py holds it to that behind a stalled stream. */
typedef struct caf_scf_desc {
    const float* d_x;       /* (rows, pitch) complex64 */
    int64_t rows, pitch, n; /* n <= pitch samples used per row */
    int32_t num_channels;   /* N' */
    int32_t hop;            /* L  */
    int32_t num_hops;       /* P  */
    int32_t conjugate;      /* 0 / 1 */
    int32_t coherence;      /* 0 / 1 */
    int32_t reserved;
    const float* d_window;  /* (N') float32, device, required */
    const float* d_smooth;  /* (P) float32, device, or NULL = ones */
    void* stream;
} caf_scf_desc;

typedef struct caf_scf_outputs { /* each optional */
    float* d_scf;                /* (rows, N', N', M)  [k + N'/2][l + N'/2][q + M/2] */
    float* d_alpha_val;          /* (rows, A) */
    int32_t* d_alpha_arg;        /* (rows, A), s of the winner */
    double* d_psd;               /* (rows, N') */
} caf_scf_outputs;

CAF_EXPORT int32_t caf_scf_fam(const caf_scf_desc* desc, const caf_scf_outputs* out);
/* m = M, num_alpha = A, min_samples = (P - 1) L + N', threads and bytes of dynamic LDS of a workgroup of the pair kernel, bytes
 * of pooled scratch per row.  Every output is optional (NULL).  Sizes that caf_scf_fam refuses: CAF_ERR_INVALID.  No device work. */
CAF_EXPORT int32_t caf_scf_geometry(int32_t num_channels, int32_t hop, int32_t num_hops, int32_t* m, int64_t* num_alpha,
                                    int64_t* min_samples, int32_t* threads, int64_t* lds_bytes, int64_t* scratch_bytes_per_row);

/* ---- any-ratio resampling of ragged batches (filterRoutines.py: resampleRows; demodulationRoutines.py: conditionBursts;
 *      caf_resample.hip).  Added without a version bump, detected by symbol. -------------------------------------------------
 * Per row r: x_r[n], complex64, valid for 0 <= n < L_r (a sample outside reads as 0); nu_r, the carrier to remove in cycles per
 * sample; t0_r, the input-sample position of output 0 (any real value); step_r > 0, input samples per output sample; w_r >= 1,
 * input samples per unit of the pulse argument; M_r >= 0, the outputs to produce.  One pulse table for the call: p[0 .. 2 H Q]
 * float32, H the half width in units, Q the entries per unit; h(u) = 0 for |u| >= H and elsewhere the linear interpolation of p
 * at position (u + H) Q.
 *   t_m    = t0_r + m step_r                                                                      (float64, one fma)
 *   y_r[m] = (1 / w_r) sum_{n : |t_m - n| < H w_r, 0 <= n < L_r} x_r[n] e^{-j 2 pi nu_r n} h((t_m - n) / w_r),   0 <= m < M_r
 *   y_r[m] = 0                                                                                     for M_r <= m < out_pitch
 * In float64 operations: H w_r is rounded once; n runs from max(floor(t_m - H w_r) + 1, 0) to min(ceil(t_m + H w_r) - 1,
 * L_r - 1); the table position is q = fma(t_m - n, Q / w_r, H Q) with Q / w_r rounded once, clamped to 0 .. 2 H Q, its entry
 * i = min(floor(q), 2 H Q - 1) and its fraction f = q - i.  In float32: the phasor (from nu_r n reduced exactly to a fraction
 * of a turn, so nu = 1e6 + 0.25 loses nothing), the mixing product, the lerp p[i] + f (p[i + 1] - p[i]), the products, the sum
 * over n upwards, and the final product with the float32 nearest 1 / w_r.
 * Limits: 1 <= H <= 16; 2 <= Q <= 1024, any integer; H Q <= 8192; 1 <= w_r <= 64; 2^-6 <= step_r <= 64; |t0_r| < 2^31;
 * |nu_r| <= 2^20; 0 <= L_r <= pitch < 2^31; 0 <= M_r <= out_pitch < 2^31; rows >= 1.  Everything else (NaN included) returns
 * CAF_ERR_INVALID with a caf_last_error() text before anything touches a device.
 * h_nu, h_t0, h_step, h_width (float64), h_lengths and h_counts (int32) are HOST arrays of `rows` entries, as the job arrays of
 * caf_kmeans_lloyd are; h_lengths may be NULL (every row has `pitch` samples).  They are checked, copied into a staging block
 * the library keeps, uploaded into a pooled block on the call's stream and given back to the pool in stream order (when an
 * event behind the launch has completed); the caller's arrays are free again on return, and no step is read from device memory
 * unchecked.  d_x (rows, pitch) and d_y (rows, out_pitch) are complex64 on the device and must not overlap; every element of
 * d_y is written.  One launch; the grid is over (row, tile of outputs) with the tile of caf_resample_geometry at the call's
 * largest step and width.  No atomics: a row gives the same bits alone or at any place in any batch, whatever the other rows'
 * steps and widths make of the tile, and on every run.  CAF_RESAMPLE_DEBUG=1 prints one line per call on stderr
 * (`[caf resample] rows=... tile=... threads=... lds=... support=...`, support = floor(2 H max w) + 1 terms).
 * The stream is a field of the descriptor: all device work of the call is queued on desc->stream and nowhere else, as for every
 * entry point that ends in `void* stream`, and the call does not wait for it; tests/test_gpu_resample.py holds it to that behind
 * a stalled stream. */
typedef struct caf_resample_desc {
    const float* d_x;         /* (rows, pitch) complex64 */
    int64_t rows, pitch;
    const int32_t* h_lengths; /* HOST (rows): L_r, or NULL = pitch */
    const double* h_nu;       /* HOST (rows): cycles per sample */
    const double* h_t0;       /* HOST (rows): input position of output 0 */
    const double* h_step;     /* HOST (rows): input samples per output */
    const double* h_width;    /* HOST (rows): input samples per unit of the pulse argument */
    const int32_t* h_counts;  /* HOST (rows): M_r */
    const float* d_table;     /* (2 H Q + 1) float32, device */
    int32_t half_width;       /* H */
    int32_t phases;           /* Q */
    float* d_y;               /* (rows, out_pitch) complex64 */
    int64_t out_pitch;
    void* stream;
} caf_resample_desc;

CAF_EXPORT int32_t caf_resample_rows(const caf_resample_desc* desc);
/* tile: the outputs of a workgroup at these sizes (a power of two up to 1024: the largest whose table and slice of
 * (tile - 1) max_step + 2 H max_width samples fit 160 KiB of LDS); threads per workgroup; bytes of dynamic LDS.  Every output is
 * optional (NULL).  Sizes that caf_resample_rows refuses: CAF_ERR_INVALID.  No device work. */
CAF_EXPORT int32_t caf_resample_geometry(int32_t half_width, int32_t phases, double max_step, double max_width, int32_t* tile,
                                         int32_t* threads, int64_t* lds_bytes);

/* ---- batched k-means and cluster scores (clusterRoutines.py: ClusterEngine, ClusterEngine2D, AngularClusterEngine;
 *      caf_cluster.hip) ---------------------------------------------------------------------------------------------------
 * Everything is float64.  d_x: (P, pitch, D) row-major, P problems of up to `pitch` points in D dimensions.  d_lengths:
 * int32 per problem, or NULL (every problem has `pitch` points; a length is clamped to 0 .. pitch).  d_mask: uint8 (P, pitch)
 * or NULL; a point is USED when it lies below its problem's length and its mask byte is not 0.  A JOB is one (problem, k)
 * pair: job_problem and job_k are HOST arrays of J int32 (checked before anything touches a device: 0 <= problem < P,
 * 1 <= k <= kmax), a restart is one more job.  Per-job arrays have a pitch of kmax: centres (J, kmax, D), counts (J, kmax).
 * Limits: 1 <= D <= 4, 1 <= kmax <= 32, 1 <= pitch <= 2^17, 1 <= J < 2^22.  Every violation returns CAF_ERR_INVALID with a
 * caf_last_error() text and no device work.  No atomics; every sum has a fixed order (the used points numbered in index
 * order, a thread taking numbers t, t + 256, ... in increasing order, lanes by xor butterfly, waves, clusters and tiles in
 * increasing order), and a job's outputs are a function of its own used points, k and centres (variates): not of J, its place
 * among the jobs, the run, the pool, the pitch, or of whether unused points are masked or absent.
 *
 * caf_kmeans_seed: k-means++ (D^2 sampling, one trial per step) from the caller's variates d_u (J, kmax) in [0, 1).  The
 * first centre is used point number floor(u_0 n_used) in index order.  For centre j >= 1: D2_i the squared distance of used
 * point i to the nearest centre chosen so far, P_i its running sum in index order (a workgroup scan per tile of 256 on top of
 * the tiles before), t = u_j P_last; chosen is the first used point with P_i > t and D2_i > 0 -- where rounding leaves none
 * the last used point with D2_i > 0, and where every used point coincides with a centre the last used point.  Outputs:
 * d_index (J, kmax) int32 point indices and d_centres (J, kmax, D), entries 0 .. k - 1 of a job.  A job with fewer used
 * points than k gets indices -1 and no centres. */
CAF_EXPORT int32_t caf_kmeans_seed(const double* d_x, int64_t P, int64_t pitch, int32_t D, const int32_t* d_lengths,
                                   const uint8_t* d_mask, const int32_t* job_problem, const int32_t* job_k, int64_t J, int32_t kmax,
                                   const double* d_u, int32_t* d_index, double* d_centres, void* stream);
/* Lloyd's iteration from d_centres (in and out), one workgroup per job, wholly on the device.  Assignment: the centre with the
 * smallest sum_d (x_d - c_d)^2, formed directly, the lower index of equal values.  Update: the mean of the members; an empty
 * cluster keeps its centre.  The job ends when an assignment repeats the labels before it (converged), or with the
 * assignment that follows update number max_iter (>= 1); either way the labels are the assignment to the centres returned.
 * Outputs: d_labels (J, pitch) int32, -1 for points not used, nothing written from the problem's length on; d_counts
 * (J, kmax) int32 and d_centres, entries 0 .. k - 1; d_inertia (J), the sum over used points of the squared distance to
 * their centre; d_n_iter (J), the updates done; d_status (J):
 *   0 converged   1 fewer used points than k: labels -1 and nothing else written   2 converged with an empty cluster
 *   3 max_iter updates done and the labels still changed (takes precedence over 2)
 * Form 1 keeps the problem's points in LDS (pitch * D * 8 <= 131072), form 2 reads them through L2 in every pass; the
 * arithmetic and its order are the same.  A single job is one workgroup however many points it has. */
CAF_EXPORT int32_t caf_kmeans_lloyd(const double* d_x, int64_t P, int64_t pitch, int32_t D, const int32_t* d_lengths,
                                    const uint8_t* d_mask, const int32_t* job_problem, const int32_t* job_k, int64_t J, int32_t kmax,
                                    int32_t max_iter, double* d_centres, int32_t* d_labels, int32_t* d_counts, double* d_inertia,
                                    int32_t* d_n_iter, int32_t* d_status, void* stream);
/* Scores of a labelling, from d_labels (label_rows, pitch) alone.  job_rows: HOST array of J int32, the row of d_labels that
 * holds a job's labels (so that the winners among restarts are scored where they lie), or NULL: row = job, label_rows is
 * ignored.  A point counts when it lies below its problem's length and its label
 * is within 0 .. k - 1; centroids are the label means.  `which` is a mask: 1 the mean silhouette (Euclidean distances formed
 * directly; a member of a singleton cluster scores 0), 2 Davies-Bouldin, 4 Calinski-Harabasz (1 when the within-cluster
 * dispersion is 0); the outputs d_sil, d_db, d_ch are (J) and required when selected.  d_sil_points (J, pitch), optional with
 * the silhouette: s(i) per counted point, NaN for the others below the length.  A job with fewer than 2 non-empty clusters,
 * or with as many non-empty clusters as points, gets NaN. */
CAF_EXPORT int32_t caf_cluster_scores(const double* d_x, int64_t P, int64_t pitch, int32_t D, const int32_t* d_lengths,
                                      const int32_t* job_problem, const int32_t* job_k, int64_t J, int32_t kmax,
                                      const int32_t* d_labels, const int32_t* job_rows, int64_t label_rows, uint32_t which,
                                      double* d_sil, double* d_db, double* d_ch, double* d_sil_points, void* stream);
/* form: 1 Lloyd with the points in LDS, 2 through L2, 0 arguments out of range; threads per workgroup; points per tile T of the
 * seeding scans and the silhouette; dynamic LDS bytes of a Lloyd workgroup and of a silhouette workgroup; pooled scratch bytes
 * per job.  Every output is optional (NULL).  No device work. */
CAF_EXPORT int32_t caf_cluster_geometry(int64_t pitch, int32_t D, int32_t kmax, int32_t* form, int32_t* threads, int32_t* tile,
                                        int64_t* lloyd_lds_bytes, int64_t* sil_lds_bytes, int64_t* scratch_bytes);

/* ---- tone spectra, the dense DFT, integer-multiple FFTs and the burst FFT (spectralRoutines.py: toneSpectrum :663-679,
 * toneSpec_kernel / toneSpecMulti_kernel :394-571, dft :637-659, IntegerMultipleFFT :128-232; burstyRoutines.py: burstFFT :14-36).
 * Added after ABI 1.10 without a version bump, detected by symbol (csrc/caf_spectral.hip).  No atomics; every sum has a fixed
 * order that depends on the row's own sizes alone, so a row of a batch holds the bits it has when run alone.  Every violation
 * (NULL, sizes below 1 or above the stated limits, fs zero or not finite, a pointer not aligned to its element) returns
 * CAF_ERR_INVALID with a caf_last_error() text before any launch.  Inputs and outputs must not overlap.  Scratch, where an
 * entry point needs any (caf_dft_rows on a cut row, caf_integer_multiple_fft with reorder), comes from the pool's owner; the tone
 * spectra and caf_burst_fft take none: they work in the caller's output.
 *
 * Tone spectra, float64 throughout: d_out (m, num_freqs) complex128,
 *   out[i][k] = -j A_i (1 - exp(-j 2 pi (f_k - f0_i) N / fs)) / (2 pi (f_k - f0_i) / fs) exp(j phi_i)
 * -- the reference's continuous-time formula, not the Dirichlet sum.  (f_k - f0_i) N / fs is reduced to a fraction of a turn before
 * the sine and cosine.  Where f_k == f0_i exactly the limit A_i N exp(j phi_i) is returned (the reference: NaN).  d_f0, d_phi,
 * d_A: m doubles each; m has no upper limit (the reference: 256).  caf_tone_spectrum_one takes the three as scalars (m = 1) and
 * runs the same kernel: its output holds the bits of the multi form's row with the same values.  1 <= N <= 2^53. */
CAF_EXPORT int32_t caf_tone_spectrum(const double* d_f0, const double* d_phi, const double* d_A, int64_t m, const double* d_freqs,
                                     int64_t num_freqs, double fs, int64_t N, double* d_out, void* stream);
CAF_EXPORT int32_t caf_tone_spectrum_one(double f0, double phi, double A, const double* d_freqs, int64_t num_freqs, double fs, int64_t N,
                                         double* d_out, void* stream);
/* out[r][k] = sum_n x[r][n] exp(-j 2 pi f_k n / fs): d_x (rows, len) complex64 (c128 = 0) or complex128 (c128 = 1), d_freqs
 * num_freqs doubles in any order and of any size, d_out (rows, num_freqs) complex128; products and sums in float64.  Pooled
 * scratch (the segments' partial sums) when len is cut: rows * segments * num_freqs complex128. */
CAF_EXPORT int32_t caf_dft_rows(const void* d_x, int32_t c128, int64_t rows, int64_t len, const double* d_freqs, int64_t num_freqs,
                                double fs, double* d_out, void* stream);
/* frequencies per workgroup T; samples per LDS chunk C; samples per Horner block R, the interval at which the phase is seeded
 * again from an exactly reduced product (the error bound grows with R, not with len); the largest len; the number of workgroups
 * per row W the cut of len aims for: with tiles = ceil(num_freqs / T) and chunks = ceil(len / C), len is cut into
 * ceil(chunks / ceil(chunks / min(chunks, ceil(W / tiles)))) segments of whole chunks, added in segment order by a second launch
 * when there is more than one.  Every output is optional (NULL).  No device work. */
CAF_EXPORT int32_t caf_dft_geometry(int32_t* freqs_per_workgroup, int32_t* samples_per_chunk, int32_t* reseed_interval, int64_t* max_len,
                                    int32_t* split_workgroups);
/* d_x (rows, len) complex64.  reorder = 0: d_out (rows, multiple, len), row i of a matrix the len-point transform of
 * x[n] exp(-j 2 pi i n / (multiple len)); reorder != 0: d_out (rows, multiple len), the transform of x zero-padded to
 * multiple len.  Three steps: the shifted copies (the phase formed from the integer i n, not by recurrence), the row transform in
 * place (complex64, rocFFT under the plan cache), and for reorder the tiled transpose (multiple, len) -> (len, multiple), for which
 * the first two steps work in pooled scratch of the output's size.  multiple * len < 2^31. */
CAF_EXPORT int32_t caf_integer_multiple_fft(const float* d_x, int64_t rows, int64_t len, int32_t multiple, int32_t reorder, float* d_out,
                                            void* stream);
/* d_x (rows, len) complex64 -> d_out (rows, length) complex64: the row zero-padded to alpha * length, alpha = ceil(len / length),
 * its alpha pieces of `length` samples added (float64, in order of the pieces, rounded once) and the sum transformed.  len < length
 * is plain zero padding. */
CAF_EXPORT int32_t caf_burst_fft(const float* d_x, int64_t rows, int64_t len, int64_t length, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CAF_H_ */
