// Batched PSK demodulation (demodulationRoutines: SimpleDemodulatorPSK / CupyDemodulatorPSK / CupyDemodulatorQPSK and the
// fused demodulateBursts).  One workgroup of 256 threads per burst (row), grid-stride over rows:
//   pass 1  the oversampled row is read once (16-byte loads) and kept in LDS DE-INTERLEAVED, phase-major:
//           sample i lives at [i % osr][i / osr], so every later read (the |x| sum of one phase, the winning phase)
//           is a unit-stride LDS read; |x| is formed in the kernel (numpy's complex absolute) and never written;
//   pass 2  moments of p = x^(m/2) (eigen form) or the sum of x^m (power-sum form) over the winning phase;
//   pass 3  rotate, map, 1 byte per symbol (reimc only when asked for);
//   then, with preambles: compare, (preamble, sample, rotation) arg max, cut / rotate / gray map, on the symbols still
//   in LDS.
// Rows that do not fit the LDS image (more than DEMOD_LDS_SAMPLES samples) take the same steps from global memory.
//
// Summation order (fixed, a function of the row alone, never of the launch): thread t of 256 adds the elements
// t, t + 256, t + 512, ... of a phase in increasing order in float32; the 64 lanes of a wave are combined by wave_sum
// (caf_wave.h: the fixed xor butterfly), the four waves as ((w0 + w1) + w2) + w3.  The stand-alone kernels and the fused
// one call the same device functions, so a chain of stand-alone calls gives the fused call's bits.
// Floating-point contraction is off in this file: every product and sum below is rounded where it is written.
#include <algorithm>
#include <cstdint>

#include "caf_internal.h"
#include "caf_wave.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int DT = 256;                     // threads per row
constexpr int DEMOD_LDS_SAMPLES = 16384;    // 128 KiB of complex64 per workgroup (+ 1 byte per symbol)
constexpr int DEMOD_MAX_OSR = 32;

// LDS of the workgroup folds of caf_wave.h: up to three sums through one barrier (a single sum uses the first field), and
// the (count, flat index) records of the arg max
struct Red {
    WaveSlots<DT / 64, float, float, float> f3;
    WaveSlots<DT / 64, uint32_t, uint32_t> u;
};

// numpy's complex absolute (the formula of k_abs_ampsq in caf_burst.hip): |x| formed here equals a precomputed abs_x bit for bit
__device__ __forceinline__ float np_abs(float2 z) {
    const float ax = fabsf(z.x), ay = fabsf(z.y);
    const float hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
    if (isinf(ax) || isinf(ay)) return INFINITY;
    if (isnan(ax) || isnan(ay)) return ax + ay;
    if (hi == 0.f) return 0.f;
    const float r = lo / hi;
    return hi * sqrtf(fmaf(r, r, 1.f));
}

__device__ __forceinline__ float2 csq(float2 a) { return make_float2(a.x * a.x - a.y * a.y, a.x * a.y + a.y * a.x); }

__constant__ float PSK8_RE[8] = {1.f, 0.70710678118654752f, 0.f, -0.70710678118654752f, -1.f, -0.70710678118654752f, 0.f,
                                 0.70710678118654752f};
__constant__ float PSK8_IM[8] = {0.f, 0.70710678118654752f, 1.f, 0.70710678118654752f, 0.f, -0.70710678118654752f, -1.f,
                                 -0.70710678118654752f};

// small tables as nibbles of one word (no scratch, no constant loads): entry i = (word >> 4 i) & 15
constexpr uint32_t MAP8_NIBBLES = 0x04261735u;   // map8[idx0][idx1][idx2] flattened: {5, 3, 7, 1, 6, 2, 4, 0}
constexpr uint32_t GRAY4_NIBBLES = 0x2013u;      // {3, 1, 0, 2}
constexpr uint32_t GRAY2_NIBBLES = 0x10u;        // {0, 1}
constexpr uint32_t ROTCHAIN_NIBBLES = 0x1302u;   // {2, 0, 3, 1}: 3 -> 1 -> 0 -> 2 -> 3

__device__ __forceinline__ uint8_t map_sym(float re, float im, int m, int map, float thr8) {
    if (map == CAF_DEMOD_MAP_SIGNBITS) {  // anticlockwise 0..3 from the sign bits (BPSK: the sign bit of re)
        const int xs = (int)(__float_as_uint(re) >> 31), ys = (int)(__float_as_uint(im) >> 31);
        if (m == 2) return (uint8_t)xs;
        return (uint8_t)(xs ? (ys ? 2 : 1) : (ys ? 3 : 0));
    }
    if (map == CAF_DEMOD_MAP_GRAYBATCH) return (uint8_t)((((__float_as_uint(re) >> 31) ^ 1u) << 1) | ((__float_as_uint(im) >> 31) ^ 1u));
    if (map == CAF_DEMOD_MAP_GENERIC) {  // arg max of the dot product with pskdicts[m], first maximum
        const int step = 8 / m;
        float best = re * PSK8_RE[0] + im * PSK8_IM[0];
        int arg = 0;
        for (int k = 1; k < m; k++) {
            const float d = re * PSK8_RE[k * step] + im * PSK8_IM[k * step];
            if (d > best) {
                best = d;
                arg = k;
            }
        }
        return (uint8_t)arg;
    }
    if (m == 2) return (uint8_t)(re < 0.f);
    if (m == 4) {  // gray4[(re > 0)][(im > 0)] = {{2, 1}, {3, 0}}
        const bool xp = re > 0.f, yp = im > 0.f;
        return (uint8_t)(xp ? (yp ? 0 : 3) : (yp ? 1 : 2));
    }
    // 8PSK: below the threshold plane the QPSK box decides, above it the diamond
    const float xmy = fabsf(re) - fabsf(im);
    const bool c1z = (fabsf(xmy) - thr8) > 0.f;
    const bool cx2 = re > 0.f, cy2 = im > 0.f, cxmy2 = xmy > 0.f;
    const bool cx3 = cxmy2 && cx2, cy3 = !cxmy2 && cy2;
    const bool idx1 = c1z ? cxmy2 : cx2;
    const bool idx2 = c1z ? (cx3 || cy3) : cy2;
    const int flat = (c1z ? 4 : 0) | (idx1 ? 2 : 0) | (idx2 ? 1 : 0);
    return (uint8_t)((MAP8_NIBBLES >> (4 * flat)) & 15u);
}

// matches[preamble][search][r] = #{ j : (preamble[j] - syms[s0 + search + j]) mod m == r } and its first arg max.
// Every index is clamped: no preamble length or search bound can read outside syms[0, nsyms) or pre[0, pre_total).
__device__ void compare_row(const uint8_t* syms, int64_t nsyms, const uint8_t* __restrict__ pre,
                            const int32_t* __restrict__ pre_len, int num_pre, int pre_total, int s0, int s1, int m,
                            uint32_t* __restrict__ matches, uint32_t& best_cnt, uint32_t& best_idx, Red& red) {
    const int S = s1 - s0;
    const int SM = S * m, mshift = m == 2 ? 1 : (m == 4 ? 2 : 3);
    uint32_t bc = 0, bi = 0xffffffffu;
    int off = 0;
    for (int p = 0; p < num_pre; p++) {
        int len = pre_len[p];
        if (len < 0) len = 0;
        if (off + len > pre_total) len = pre_total > off ? pre_total - off : 0;
        for (int i = threadIdx.x; i < SM; i += DT) {
            const int s = i >> mshift, r = i & (m - 1);
            const int64_t base = (int64_t)s0 + s;
            uint32_t cnt = 0;
            for (int j = 0; j < len; j++) {
                const int64_t k = base + j;
                if (k >= 0 && k < nsyms) cnt += ((((int)pre[off + j] - (int)syms[k]) & (m - 1)) == r) ? 1u : 0u;
            }
            const uint32_t flat = (uint32_t)(p * SM + i);
            if (matches) matches[flat] = cnt;
            if (first_max(bc, bi, cnt, flat)) {
                bc = cnt;
                bi = flat;
            }
        }
        off += len;
    }
    block_argmax_all(red.u, bc, bi);
    best_cnt = bc;
    best_idx = bi;
}

// out[t] = gray[(syms[offset + t] + rotation) mod m], t < stop - offset, inside both rows; count = stop - offset
__device__ void cut_row(const uint8_t* syms, int64_t nsyms, uint32_t key_len, uint32_t sample, uint32_t rotation, uint32_t stop,
                        int m, int64_t out_length, uint8_t* __restrict__ out, uint32_t* __restrict__ count) {
    const uint32_t offset = key_len + sample;
    const int32_t total = (int32_t)(stop - offset);
    if (total < 0) return;
    const uint32_t gray = m == 2 ? GRAY2_NIBBLES : GRAY4_NIBBLES;
    for (int32_t t = threadIdx.x; t < total; t += DT) {
        const int64_t k = (int64_t)offset + t;
        if (t < out_length && k < nsyms) out[t] = (uint8_t)((gray >> (4 * ((syms[k] + rotation) & (uint32_t)(m - 1)))) & 15u);
    }
    if (threadIdx.x == 0 && count) *count = (uint32_t)total;
}

struct RowCtx {
    const float2* xr;   // the row in global memory
    const float2* s_x;  // its phase-major LDS image (LDS rows only)
    int64_t nsym;
    int osr;
};

template <bool LDS>
__device__ __forceinline__ float2 sample_of(const RowCtx& c, int ph, int64_t s) {
    if constexpr (LDS) return c.s_x[(int64_t)ph * c.nsym + s];
    else return c.xr[s * c.osr + ph];
}

// eye opening of one row: the osr phase sums of |x| (or of the given abs), first maximum
template <bool LDS>
__device__ void eye_row(const RowCtx& c, const float* __restrict__ absr, float* s_acc, float* __restrict__ eo_metric, int& best_ph,
                        float& best_sum, Red& red) {
    const int osr = c.osr;
    if (!LDS && !absr) {
        // one pass over the row: per-thread, per-phase accumulators in LDS see the additions of the per-phase loop, in its order
        for (int ph = 0; ph < osr; ph++) s_acc[ph * DT + threadIdx.x] = 0.f;
        for (int64_t s = threadIdx.x; s < c.nsym; s += DT)
            for (int ph = 0; ph < osr; ph++) s_acc[ph * DT + threadIdx.x] += np_abs(c.xr[s * osr + ph]);
    }
    int bp = 0;
    float bs = 0.f;
    for (int ph = 0; ph < osr; ph++) {
        float acc = 0.f;
        if (absr) {
            for (int64_t s = threadIdx.x; s < c.nsym; s += DT) acc += absr[s * osr + ph];
        } else if constexpr (LDS) {
            for (int64_t s = threadIdx.x; s < c.nsym; s += DT) acc += np_abs(c.s_x[(int64_t)ph * c.nsym + s]);
        } else {
            acc = s_acc[ph * DT + threadIdx.x];
        }
        const float sum = block_sum_all(acc, red.f3.a);
        if (eo_metric && threadIdx.x == 0) eo_metric[ph] = sum;
        if (ph == 0 || sum > bs) {  // the first maximum wins
            bp = ph;
            bs = sum;
        }
    }
    best_ph = bp;
    best_sum = bs;
}

struct DemodKernelArgs {
    caf_demod_desc d;
    int lds_samples;  // capacity of the LDS image in samples (0: no image, every row from global memory)
    int lds_syms;     // capacity of the LDS symbol buffer
};

template <bool LDS>
__device__ void demod_row(const DemodKernelArgs& a, int64_t row, int m, int64_t n_valid, float2* s_x, uint8_t* s_sym, Red& red) {
    const caf_demod_desc& d = a.d;
    const int osr = d.osr;
    const int64_t nsym = n_valid / osr, pitch = d.xlength / osr;
    const float2* xr = (const float2*)d.d_x + row * d.xlength;
    RowCtx c{xr, s_x, nsym, osr};
    const int64_t n = nsym * osr;

    if constexpr (LDS) {
        // pass 1: 16-byte loads where the row allows them, de-interleaved on the way into LDS
        const int n32 = (int)n, ns32 = (int)nsym;  // (an LDS row: n <= DEMOD_LDS_SAMPLES)
        if ((((uintptr_t)xr) & 15) == 0) {
            const float4* xv = (const float4*)xr;
            for (int i = 2 * (int)threadIdx.x; i < n32; i += 2 * DT) {
                if (i + 1 < n32) {
                    const float4 v = xv[i >> 1];
                    s_x[(i % osr) * ns32 + i / osr] = make_float2(v.x, v.y);
                    s_x[((i + 1) % osr) * ns32 + (i + 1) / osr] = make_float2(v.z, v.w);
                } else {
                    s_x[(i % osr) * ns32 + i / osr] = xr[i];
                }
            }
        } else {
            for (int i = threadIdx.x; i < n32; i += DT) s_x[(i % osr) * ns32 + i / osr] = xr[i];
        }
        __syncthreads();
    }

    int ph = 0;
    float best_sum = 0.f;
    eye_row<LDS>(c, d.d_abs ? d.d_abs + row * d.xlength : nullptr, (float*)s_x, d.d_eo_metric ? d.d_eo_metric + row * osr : nullptr, ph,
                 best_sum, red);
    if (threadIdx.x == 0 && d.d_eo_index) d.d_eo_index[row] = ph;
    if (d.d_xeo) {  // the winning phase, copied (complex64, not computed)
        float2* xo = (float2*)d.d_xeo + row * d.xeo_pitch;
        for (int64_t s = threadIdx.x; s < nsym; s += DT) xo[s] = sample_of<LDS>(c, ph, s);
    }
    if (d.eye_only) return;

    // pass 2: phase lock
    const int powerup = m >> 1;  // p = x^(m/2): BPSK x, QPSK x^2, 8PSK x^4
    float angle, metric = 0.f, s00 = 0.f, s01 = 0.f, s11 = 0.f;
    if (d.lock == CAF_DEMOD_LOCK_EIG) {
        for (int64_t s = threadIdx.x; s < nsym; s += DT) {
            float2 p = sample_of<LDS>(c, ph, s);
            if (powerup >= 2) p = csq(p);
            if (powerup >= 4) p = csq(p);
            s00 += p.x * p.x;
            s01 += p.x * p.y;
            s11 += p.y * p.y;
        }
        block_sum_all(red.f3, s00, s01, s11);
        // S = [s00 s01; s01 s11]: l1,2 = T / 2 +- sqrt(h^2 + s01^2), h = (s00 - s11) / 2.  The leading eigenvector is
        // (l1 - s11, s01) = (h + r, s01); for h < 0 that difference cancels, so its parallel (s01, l1 - s00) = (s01, r - h) is used,
        // with the sign that keeps the first component >= 0 (the sign rule of the closed form).  s01 == 0 and l1 == s11: pi / 2
        // when s11 > s00, 0 when the matrix is a multiple of the identity.
        const float h = 0.5f * (s00 - s11), r = sqrtf(h * h + s01 * s01), t2 = 0.5f * (s00 + s11);
        const float l1 = t2 + r;
        float l2 = t2 - r;
        if (l2 < 0.f) l2 = 0.f;
        float v0, v1;
        if (h >= 0.f) {
            v0 = h + r;
            v1 = s01;
        } else {
            v0 = fabsf(s01);
            v1 = s01 < 0.f ? -(r - h) : (r - h);
        }
        angle = atan2f(v1, v0);
        metric = l1 > 0.f ? l2 / l1 : 0.f;
    } else if (d.lock == CAF_DEMOD_LOCK_NONE) {
        angle = 0.f;
    } else {
        float sr = 0.f, si = 0.f, z = 0.f;  // (z: the record's third field, unused here)
        for (int64_t s = threadIdx.x; s < nsym; s += DT) {
            float2 p = csq(sample_of<LDS>(c, ph, s));
            if (m >= 4) p = csq(p);
            if (m >= 8) p = csq(p);
            sr += p.x;
            si += p.y;
        }
        block_sum_all(red.f3, sr, si, z);
        angle = atan2f(si, sr);
        s00 = sr;
        s01 = si;
    }
    if (threadIdx.x == 0) {
        if (d.d_angle) d.d_angle[row] = angle;
        if (d.d_svd) d.d_svd[row] = metric;
        if (d.d_moments) {
            d.d_moments[row * 3 + 0] = s00;
            d.d_moments[row * 3 + 1] = s01;
            d.d_moments[row * 3 + 2] = s11;
        }
    }

    // pass 3: rotate and map
    const float div = d.lock == CAF_DEMOD_LOCK_EIG ? (float)powerup : (float)m;
    float phi = -angle / div;
    if (m == 4 && d.map != CAF_DEMOD_MAP_GENERIC && d.lock != CAF_DEMOD_LOCK_NONE) phi += 0.78539816339744831f;  // to the box of the sign comparators
    float sn, cs;
    sincosf(phi, &sn, &cs);
    if (d.lock == CAF_DEMOD_LOCK_NONE) {
        sn = 0.f;
        cs = 1.f;
    }
    const float thr8 = 0.54119610014619698f * (d.scaling > 0.f ? d.scaling : (nsym > 0 ? best_sum / (float)nsym : 0.f));  // |cos(pi/8) - sin(pi/8)| max(eo mean)
    uint8_t* so = d.d_syms + row * pitch;
    float2* ro = d.d_reimc ? (float2*)d.d_reimc + row * pitch : nullptr;
    for (int64_t s = threadIdx.x; s < nsym; s += DT) {
        const float2 x = sample_of<LDS>(c, ph, s);
        const float re = x.x * cs - x.y * sn, im = x.x * sn + x.y * cs;
        const uint8_t sym = map_sym(re, im, m, d.map, thr8);
        so[s] = sym;
        if (LDS && s < a.lds_syms) s_sym[s] = sym;
        if (ro) ro[s] = make_float2(re, im);
    }

    if (d.num_preambles <= 0 || m == 8) return;  // (cut / rotate has no gray map for 8PSK)
    __syncthreads();  // the symbols are complete (LDS, or this workgroup's own global writes)
    const uint8_t* sy = (LDS && nsym <= a.lds_syms) ? (const uint8_t*)s_sym : (const uint8_t*)so;
    uint32_t bc, bi;
    compare_row(sy, nsym, d.d_preambles, d.d_preamble_lengths, d.num_preambles, d.preamble_total, d.search_start, d.search_end, m,
                nullptr, bc, bi, red);
    const int S = d.search_end - d.search_start;
    const uint32_t A = bi / (uint32_t)(S * m), rem = bi - A * (uint32_t)(S * m);
    const uint32_t B = rem / (uint32_t)m, C = rem - B * (uint32_t)m;
    const uint32_t sample = (uint32_t)d.search_start + B;
    if (threadIdx.x == 0 && d.d_best) {
        d.d_best[row * 4 + 0] = A;
        d.d_best[row * 4 + 1] = sample;
        d.d_best[row * 4 + 2] = C;
        d.d_best[row * 4 + 3] = bc;
    }
    if (d.d_payload) {
        int32_t kl = A < (uint32_t)d.num_preambles ? d.d_preamble_lengths[A] : 0;
        if (kl < 0) kl = 0;
        cut_row(sy, nsym, (uint32_t)kl, sample, C, (uint32_t)nsym, m, d.out_length, d.d_payload + row * d.out_length,
                d.d_count ? d.d_count + row : nullptr);
    }
}

__global__ __launch_bounds__(DT) void k_psk_demod_rows(const DemodKernelArgs a) {
    extern __shared__ float4 s_dyn[];
    __shared__ Red red;
    float2* s_x = (float2*)s_dyn;
    uint8_t* s_sym = (uint8_t*)(s_x + a.lds_samples);
    const caf_demod_desc& d = a.d;
    for (int64_t row = blockIdx.x; row < d.rows; row += gridDim.x) {
        const int m = d.d_m ? (int)d.d_m[row] : d.m;
        if (!d.eye_only && m != 2 && m != 4 && m != 8) continue;  // a row of another order: untouched
        if (!d.eye_only && m == 8 && d.map >= CAF_DEMOD_MAP_SIGNBITS) continue;  // (the sign-bit maps know BPSK and QPSK)
        int64_t n_valid = d.xlength;
        if (d.d_lengths) {
            const int64_t l = d.d_lengths[row];
            n_valid = l < 0 ? 0 : (l < d.xlength ? l : d.xlength);
        }
        const int64_t n = (n_valid / d.osr) * d.osr;
        if (n <= a.lds_samples) demod_row<true>(a, row, m, n_valid, s_x, s_sym, red);
        else demod_row<false>(a, row, m, n_valid, s_x, s_sym, red);
        __syncthreads();  // the LDS image goes to the next row
    }
}

// the same eye-opening steps alone (getEyeOpening_batch): phase sums, first maximum, the winning phase copied out
__global__ __launch_bounds__(DT) void k_eye_opening_batch(const DemodKernelArgs a) {
    extern __shared__ float4 s_dyn[];
    __shared__ Red red;
    float2* s_x = (float2*)s_dyn;
    const caf_demod_desc& d = a.d;
    for (int64_t row = blockIdx.x; row < d.rows; row += gridDim.x) {
        const int64_t n = (d.xlength / d.osr) * d.osr;
        if (n <= a.lds_samples) demod_row<true>(a, row, 0, d.xlength, s_x, nullptr, red);
        else demod_row<false>(a, row, 0, d.xlength, s_x, nullptr, red);
        __syncthreads();
    }
}

__global__ __launch_bounds__(DT) void k_compare_int_preambles(const uint8_t* __restrict__ syms, int64_t rows, int64_t syms_length,
                                                              int s0, int s1, const uint8_t* __restrict__ pre, int pre_total,
                                                              const int32_t* __restrict__ pre_len, int num_pre, int m,
                                                              const uint8_t* __restrict__ mask, uint32_t* __restrict__ matches) {
    __shared__ Red red;
    const int64_t per_row = (int64_t)num_pre * (s1 - s0) * m;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        if (mask && (int)mask[row] != m) continue;  // rows of another order stay zero
        uint32_t bc, bi;
        compare_row(syms + row * syms_length, syms_length, pre, pre_len, num_pre, pre_total, s0, s1, m, matches + row * per_row, bc,
                    bi, red);
    }
}

__global__ __launch_bounds__(DT) void k_cut_rotate_gray(const uint32_t* __restrict__ index, int64_t rows,
                                                        const uint8_t* __restrict__ syms, int64_t syms_length,
                                                        const uint32_t* __restrict__ key_len, int num_keys,
                                                        const uint32_t* __restrict__ stops, int m, int64_t out_length,
                                                        uint8_t* __restrict__ out, uint32_t* __restrict__ count,
                                                        const uint8_t* __restrict__ mask) {
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        if (mask && (int)mask[row] != m) continue;
        const uint32_t A = index[row * 3 + 0];
        if (A >= (uint32_t)num_keys) continue;  // no such key: the row is left alone
        cut_row(syms + row * syms_length, syms_length, key_len[A], index[row * 3 + 1], index[row * 3 + 2], stops[row], m, out_length,
                out + row * out_length, count ? count + row : nullptr);
    }
}

// the amble search of CupyDemodulatorQPSK._demodBatch on gray symbols ((re >= +0) << 1 | (im >= +0)): per search index the best
// of the four rotations (chain 3 -> 1 -> 0 -> 2 -> 3, first maximum), the best index (first maximum), the symbols rotated by
// it as uint32, then bitslen unpacked bits, MSB first, two per symbol, from search_start + best index + amble length.
__global__ __launch_bounds__(DT) void k_amble_search_bits(const uint8_t* __restrict__ syms, int64_t rows, int64_t L,
                                                          const int32_t* __restrict__ amble, int amble_len, int search_start,
                                                          int search_len, uint32_t* __restrict__ syms_out,
                                                          int32_t* __restrict__ best_matches, int32_t* __restrict__ best_rot,
                                                          int32_t* __restrict__ best_idx, uint8_t* __restrict__ bits, int64_t bitslen) {
    __shared__ Red red;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint8_t* sy = syms + row * L;
        uint32_t bc = 0, bi = 0xffffffffu;
        for (int i = threadIdx.x; i < search_len; i += DT) {
            uint32_t cnt[4] = {0, 0, 0, 0};
            for (int j = 0; j < amble_len; j++) {
                const int64_t k = (int64_t)search_start + i + j;
                if (k < 0 || k >= L) continue;
                uint32_t sym = sy[k] & 3u;
                const int32_t want = amble[j];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (r) sym = (ROTCHAIN_NIBBLES >> (4 * sym)) & 15u;
                    cnt[r] += ((int32_t)sym == want) ? 1u : 0u;
                }
            }
            uint32_t rot = 0, best = cnt[0];
#pragma unroll
            for (int r = 1; r < 4; r++)
                if (cnt[r] > best) {
                    best = cnt[r];
                    rot = r;
                }
            const uint32_t flat = (uint32_t)i * 4u + rot;  // (one candidate per search index: its best rotation)
            if (first_max(bc, bi, best, flat)) {
                bc = best;
                bi = flat;
            }
        }
        block_argmax_all(red.u, bc, bi);
        const int idx = (int)(bi >> 2), rot = (int)(bi & 3u);
        if (threadIdx.x == 0) {
            best_matches[row] = (int32_t)bc;
            best_rot[row] = rot;
            best_idx[row] = idx;
        }
        for (int64_t s = threadIdx.x; s < L; s += DT) {
            uint32_t sym = sy[s] & 3u;
            for (int r = 0; r < rot; r++) sym = (ROTCHAIN_NIBBLES >> (4 * sym)) & 15u;
            syms_out[row * L + s] = sym;
        }
        const int64_t start = (int64_t)search_start + idx + amble_len;
        for (int64_t b = threadIdx.x; b < bitslen / 2; b += DT) {
            const int64_t k = start + b;
            uint32_t sym = 0;
            if (k < L) {  // (a symbol past the row reads as 0)
                sym = sy[k] & 3u;
                for (int r = 0; r < rot; r++) sym = (ROTCHAIN_NIBBLES >> (4 * sym)) & 15u;
            }
            bits[row * bitslen + 2 * b] = (uint8_t)((sym >> 1) & 1u);
            bits[row * bitslen + 2 * b + 1] = (uint8_t)(sym & 1u);
        }
    }
}

unsigned rows_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(rows, 1 << 16)); }

int launch_demod(const caf_demod_desc& d, bool eye_kernel, hipStream_t st) {
    DemodKernelArgs a;
    a.d = d;
    const int64_t n = (d.xlength / d.osr) * d.osr;
    // the image of a whole row where it fits; with per-row lengths a long matrix may still hold short rows; otherwise only the
    // osr * 256 float accumulators of the global-memory path
    if (n <= DEMOD_LDS_SAMPLES) a.lds_samples = (int)n;
    else if (d.d_lengths) a.lds_samples = DEMOD_LDS_SAMPLES;
    else a.lds_samples = d.osr * DT / 2;
    a.lds_syms = eye_kernel ? 0 : (int)std::min<int64_t>(a.lds_samples, d.xlength / d.osr);
    const size_t bytes = (size_t)a.lds_samples * 8 + (size_t)a.lds_syms + 16;
    const void* fn = eye_kernel ? (const void*)k_eye_opening_batch : (const void*)k_psk_demod_rows;
    if (const int rc = allow_dynamic_lds(fn, bytes)) return rc;
    if (eye_kernel) hipLaunchKernelGGL(k_eye_opening_batch, dim3(rows_grid(d.rows)), dim3(DT), bytes, st, a);
    else hipLaunchKernelGGL(k_psk_demod_rows, dim3(rows_grid(d.rows)), dim3(DT), bytes, st, a);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int check_desc(const caf_demod_desc* d, bool eye) {
    CAF_REQUIRE(d != nullptr, "caf demod: NULL descriptor");
    CAF_REQUIRE(d->rows >= 0 && d->xlength >= 1, "caf demod: rows must be >= 0 and xlength >= 1");
    CAF_REQUIRE(d->osr >= 1 && d->osr <= DEMOD_MAX_OSR, "caf demod: osr must be in [1, 32]");
    CAF_REQUIRE(d->xlength / d->osr >= 1, "caf demod: the row is shorter than one symbol");
    CAF_REQUIRE(d->xlength <= ((int64_t)1 << 31) - 1, "caf demod: xlength must be < 2^31");
    if (d->rows == 0) return CAF_OK;
    CAF_REQUIRE(d->d_x != nullptr, "caf demod: NULL input");
    if (eye) {
        CAF_REQUIRE(d->d_xeo == nullptr || d->xeo_pitch >= d->xlength / d->osr, "caf_eye_opening_batch: d_xeo rows are too short");
        return CAF_OK;
    }
    CAF_REQUIRE(d->d_syms != nullptr, "caf_psk_demod_rows: NULL d_syms");
    CAF_REQUIRE(d->d_m != nullptr || d->m == 2 || d->m == 4 || d->m == 8, "caf_psk_demod_rows: m must be 2, 4 or 8 (or per row in d_m)");
    CAF_REQUIRE(d->lock >= CAF_DEMOD_LOCK_EIG && d->lock <= CAF_DEMOD_LOCK_NONE, "caf_psk_demod_rows: unknown lock");
    CAF_REQUIRE(d->map >= CAF_DEMOD_MAP_CLASS && d->map <= CAF_DEMOD_MAP_GRAYBATCH, "caf_psk_demod_rows: unknown map");
    CAF_REQUIRE(d->d_xeo == nullptr || d->xeo_pitch >= d->xlength / d->osr, "caf_psk_demod_rows: d_xeo rows are too short");
    if (d->num_preambles > 0) {
        CAF_REQUIRE(d->d_preambles && d->d_preamble_lengths, "caf_psk_demod_rows: NULL preambles");
        CAF_REQUIRE(d->preamble_total >= 1 && d->max_preamble_length >= 1 && d->max_preamble_length <= d->preamble_total,
                    "caf_psk_demod_rows: preamble lengths");
        CAF_REQUIRE(d->search_start >= 0 && d->search_end > d->search_start, "caf_psk_demod_rows: search range");
        CAF_REQUIRE((int64_t)d->search_end + d->max_preamble_length - 1 <= d->xlength / d->osr,
                    "caf_psk_demod_rows: the search extends past the symbols");
        CAF_REQUIRE((int64_t)d->num_preambles * (d->search_end - d->search_start) * 8 < ((int64_t)1 << 31),
                    "caf_psk_demod_rows: too many (preamble, search) pairs");
        CAF_REQUIRE(d->d_payload == nullptr || d->out_length >= 1, "caf_psk_demod_rows: out_length");
    }
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_psk_demod_rows(const caf_demod_desc* desc, void* stream) {
    if (const int rc = check_desc(desc, false)) return rc;
    if (desc->rows == 0) return CAF_OK;
    caf_demod_desc d = *desc;
    d.eye_only = 0;
    return launch_demod(d, false, (hipStream_t)stream);
}

int32_t caf_eye_opening_batch(const float* d_abs, const float* d_x, int64_t rows, int64_t xlength, int32_t osr, float* d_xeo,
                              int64_t xeo_pitch, int32_t* d_eo_index, float* d_eo_metric, void* stream) {
    caf_demod_desc d = {};
    d.d_x = d_x;
    d.rows = rows;
    d.xlength = xlength;
    d.osr = osr;
    d.d_abs = d_abs;
    d.d_xeo = d_xeo;
    d.xeo_pitch = xeo_pitch;
    d.d_eo_index = d_eo_index;
    d.d_eo_metric = d_eo_metric;
    d.eye_only = 1;
    if (const int rc = check_desc(&d, true)) return rc;
    if (rows == 0) return CAF_OK;
    return launch_demod(d, true, (hipStream_t)stream);
}

int32_t caf_compare_int_preambles(const uint8_t* d_syms, int64_t rows, int64_t syms_length, int32_t search_start, int32_t search_end,
                                  const uint8_t* d_preambles, int32_t preamble_total, const int32_t* d_preamble_lengths,
                                  int32_t num_preambles, int32_t max_preamble_length, int32_t m, const uint8_t* d_psk_m,
                                  uint32_t* d_matches, void* stream) {
    CAF_REQUIRE(m == 2 || m == 4 || m == 8, "caf_compare_int_preambles: m must be 2/4/8");
    CAF_REQUIRE(rows >= 0 && syms_length >= 1, "caf_compare_int_preambles: shape");
    CAF_REQUIRE(num_preambles >= 1 && preamble_total >= 1 && max_preamble_length >= 1 && max_preamble_length <= preamble_total,
                "caf_compare_int_preambles: preamble lengths");
    CAF_REQUIRE(search_start >= 0 && search_end > search_start, "caf_compare_int_preambles: search range");
    CAF_REQUIRE((int64_t)search_end + max_preamble_length - 1 <= syms_length, "caf_compare_int_preambles: the search extends past the symbols");
    CAF_REQUIRE((int64_t)num_preambles * (search_end - search_start) * m < ((int64_t)1 << 31), "caf_compare_int_preambles: too many pairs");
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_syms && d_preambles && d_preamble_lengths && d_matches, "caf_compare_int_preambles: NULL buffer");
    hipLaunchKernelGGL(k_compare_int_preambles, dim3(rows_grid(rows)), dim3(DT), 0, (hipStream_t)stream, d_syms, rows, syms_length,
                       search_start, search_end, d_preambles, preamble_total, d_preamble_lengths, num_preambles, m, d_psk_m, d_matches);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_cut_rotate_gray(const uint32_t* d_index, int64_t rows, const uint8_t* d_syms, int64_t syms_length,
                            const uint32_t* d_key_lengths, int32_t num_keys, const uint32_t* d_sample_stops, int32_t m,
                            int64_t out_length, uint8_t* d_out, uint32_t* d_count, const uint8_t* d_psk_m, void* stream) {
    CAF_REQUIRE(m == 2 || m == 4, "caf_cut_rotate_gray: the gray maps are defined for m = 2 and m = 4");
    CAF_REQUIRE(rows >= 0 && syms_length >= 1 && out_length >= 1 && num_keys >= 1, "caf_cut_rotate_gray: shape");
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_index && d_syms && d_key_lengths && d_sample_stops && d_out, "caf_cut_rotate_gray: NULL buffer");
    hipLaunchKernelGGL(k_cut_rotate_gray, dim3(rows_grid(rows)), dim3(DT), 0, (hipStream_t)stream, d_index, rows, d_syms, syms_length,
                       d_key_lengths, num_keys, d_sample_stops, m, out_length, d_out, d_count, d_psk_m);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_amble_search_bits(const uint8_t* d_syms, int64_t rows, int64_t syms_length, const int32_t* d_amble, int32_t amble_length,
                              int32_t search_start, int32_t search_length, uint32_t* d_syms_out, int32_t* d_best_matches,
                              int32_t* d_best_rotations, int32_t* d_best_idx, uint8_t* d_bits, int64_t bits_length, void* stream) {
    CAF_REQUIRE(rows >= 0 && syms_length >= 1, "caf_amble_search_bits: shape");
    CAF_REQUIRE(amble_length >= 1 && search_start >= 0 && search_length >= 1 && bits_length >= 0, "caf_amble_search_bits: arguments");
    CAF_REQUIRE((int64_t)search_start + search_length - 1 + amble_length <= syms_length,
                "caf_amble_search_bits: the search extends past the row");
    CAF_REQUIRE(search_length < (1 << 29), "caf_amble_search_bits: search_length");
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_syms && d_amble && d_syms_out && d_best_matches && d_best_rotations && d_best_idx && (d_bits || bits_length < 2),
                "caf_amble_search_bits: NULL buffer");
    hipLaunchKernelGGL(k_amble_search_bits, dim3(rows_grid(rows)), dim3(DT), 0, (hipStream_t)stream, d_syms, rows, syms_length, d_amble,
                       amble_length, search_start, search_length, d_syms_out, d_best_matches, d_best_rotations, d_best_idx, d_bits,
                       bits_length);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
