// CFAR detection on CAF surfaces (xcorrRoutines.py: cfarDetect): a threshold that follows the local floor, and a list of the cells
// above it.  For the cell (i, j) of a map with v = S[i, j] = d_surface[i stride_d + j stride_f] (include/caf.h has the definition):
//   ring    the cells (i + a, j + b), |a| <= Hd, |b| <= Hf, outside the guard box |a| <= gd and |b| <= gf, inside the map (the
//           column modulo nf with wrap_f), finite;  Hd = gd + td, Hf = gf + tf
//   noise   CA: R / n over the ring;  GO / SO: the larger / smaller of R_A / n_A and R_B / n_B over the halves of negative and
//           positive offset on split_axis
//   a detection: v finite, n >= min_cells, v >= floor, v > alpha noise, and v the first maximum of its (2 md + 1) x (2 mf + 1) window.
//
//   k_cfar<false>      one workgroup of CFAR_T = 256 per CFAR_TILE x CFAR_TILE = 32 x 32 cells of one map.  The tile and its halo
//                      (max(Hd, 1) rows and max(Hf, 1) columns on each side, NaN outside the map) go to LDS as float32, read along
//                      whichever axis has stride +-1.  Pass 1, along f, for every row of the halo and every column of the tile: the
//                      four sums Lo = sum_{-Hf <= b < -gf}, Li = sum_{-gf <= b < 0}, Ri = sum_{0 < b <= gf}, Ro = sum_{gf < b <= Hf},
//                      each from its first b upwards, and La = Lo + Li, Ra = Ri + Ro with their cell counts.  With whole rows (CA
//                      and a split on delay) it keeps T = (La + Ra) + centre and T' = Lo + Ro, two sums per (row, column), else
//                      Lo, La, Ro, Ra.  Pass 2, along d, for every cell: with T(a) = T for |a| > gd and T' otherwise,
//                        split on delay (and CA):  A = sum_{a < 0} T(a),  B = sum_{a > 0} T(a),  Z = T(0), each from its first a upwards;
//                        split on frequency:       A = sum_a (|a| > gd ? La : Lo),  B = sum_a (|a| > gd ? Ra : Ro),  a from -Hd upwards;
//                        CA: R = (A + B) + Z.
//                      A ring value therefore passes at most Hf + 2 Hd + 6 additions: tests/cfar_ref.py forms its bound from that.
//                      It writes the noise map and, per row of the tile (a segment), the number of detections.
//   k_cfar_segscan     the segments, laid out in the order of the list (map, row, tile column), scanned 1024 at a time; the
//   launch_scan_exclusive   chunks' totals scanned by one workgroup; k_cfar_counts: the maps' totals.
//   k_cfar<true>       the same arithmetic once more in the tiles that hold a detection below cap, each record to its place.
// Count, scan, fill: no atomics, the list is a function of the data alone.  Every load of a surface is predicated on
// 0 <= i < nd and 0 <= j < nf, offsets are int64.  The maps (a host array, checked here first), the segment counts and their
// scans ride the call's stream in one pooled block behind an event (caf_lane.h).  The call waits for nothing and reads no count.
// Floating-point contraction is off in this file.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "caf_internal.h"
#include "caf_lane.h"
#include "caf_wave.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int CFAR_T = 256;      // threads per workgroup
constexpr int CFAR_TILE = 32;    // cells per tile and axis
constexpr int CFAR_CPT = CFAR_TILE * CFAR_TILE / CFAR_T;  // cells per thread
constexpr int CFAR_HMAX = 32;    // the largest half width
constexpr int CFAR_CHUNK = 1024; // segments per workgroup of the first scan
constexpr int64_t CFAR_MAX_B = (int64_t)1 << 20;
constexpr int64_t CFAR_LDS_BUDGET = 160 * 1024;

// a map as the kernels read it, B + 1 of them: the last holds the totals
struct CfarMap {
    const float* s;
    float* noise;
    int64_t sd, sf;
    int32_t nd, nf;
    int32_t ntf, pad;     // tile columns
    int64_t tile0, seg0;  // the map's first workgroup and first segment
    double alpha, floor;
};
static_assert(sizeof(CfarMap) == 80, "CfarMap is ten 8-byte words");

struct CfarArgs {
    const CfarMap* maps;
    int32_t B, gd, gf, Hd, Hf, md, mf, mode, split, wrap, min_cells;
    int32_t* cnt;          // (segments) detections per segment
    const int32_t* loc;    // (segments) exclusive scan within the chunk
    const int64_t* cbase;  // (chunks + 1) exclusive scan of the chunks' totals
    caf_cfar_det* det;
    int64_t cap;
};

constexpr int cfar_halo(int H) { return H > 1 ? H : 1; }
// LDS of a workgroup: `sums` float64 sums (two when the rows are whole: CA and a split on delay; four for a split on frequency)
// and their packed counts per (row of the halo, column of the tile), then the float32 tile
constexpr int64_t cfar_lds(int Hd, int Hf, int sums = 4) {
    const int64_t RH = CFAR_TILE + 2 * cfar_halo(Hd), RW = (CFAR_TILE + 2 * cfar_halo(Hf)) | 1;
    return RH * CFAR_TILE * (sums * 8 + 4) + RH * RW * 4;
}

// the number of detections before segment s of the call (s = the number of segments: all of them)
__device__ __forceinline__ int64_t cfar_before(const CfarArgs& a, int64_t s, int64_t nseg) {
    return s < nseg ? a.cbase[s / CFAR_CHUNK] + a.loc[s] : a.cbase[(nseg + CFAR_CHUNK - 1) / CFAR_CHUNK];
}

// (adding 0.0 changes no bit of a sum that starts at +0.0: the loops stay free of branches)
__device__ __forceinline__ void cfar_add(float x, double& s, uint32_t& n) {
    const bool f = std::isfinite(x);
    s += f ? (double)x : 0.0;
    n += f ? 1u : 0u;
}

// the vertex of the parabola through (-1, p), (0, v), (1, q) where it is a maximum, clamped to half a cell
__device__ __forceinline__ float cfar_subcell(float pf, float vf, float qf) {
    if (!std::isfinite(pf) || !std::isfinite(qf)) return 0.f;
    const double p = pf, v = vf, q = qf;
    const double den = (p - 2.0 * v) + q;
    if (!(den < 0.0)) return 0.f;
    const double d = (0.5 * (p - q)) / den;
    return (float)fmin(fmax(d, -0.5), 0.5);
}

template <bool FILL>
__global__ __launch_bounds__(CFAR_T) void k_cfar(const CfarArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    __shared__ int32_t s_w[CFAR_T / 64];
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    int lo = 0, hi = a.B;  // maps[lo].tile0 <= blk < maps[hi].tile0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.maps[mid].tile0 <= blk) lo = mid;
        else hi = mid;
    }
    const CfarMap m = a.maps[lo];
    const int64_t nseg = a.maps[a.B].seg0;
    const int64_t t = blk - m.tile0;
    const int64_t ti = t / m.ntf;
    const int tj = (int)(t - ti * m.ntf);
    const int64_t seg_row0 = m.seg0 + ti * CFAR_TILE * (int64_t)m.ntf + tj;  // the segment of the tile's row r: + r ntf

    if constexpr (FILL) {  // nothing to write: no detection in the tile, or all of them past cap
        int32_t c = 0;
        if (tid < CFAR_TILE) {
            const int64_t seg = seg_row0 + (int64_t)tid * m.ntf;
            c = a.cnt[seg];
            if (c && cfar_before(a, seg, nseg) - cfar_before(a, m.seg0, nseg) >= a.cap) c = 0;
        }
        if (block_sum(c, s_w) == 0) return;
    }

    const int Hd = a.Hd, Hf = a.Hf, gd = a.gd, gf = a.gf;
    const int hd = Hd > 1 ? Hd : 1, hf = Hf > 1 ? Hf : 1;
    const int RH = CFAR_TILE + 2 * hd, RW = CFAR_TILE + 2 * hf, RWp = RW | 1;
    const bool rows_whole = a.mode == CAF_CFAR_CA || a.split == 0;  // T(a) is formed in pass 1: two sums per (row, column), else four
    double* s_lo = reinterpret_cast<double*>(s_dyn);                // rows_whole: T(a) of a row outside the guard rows
    double* s_la = s_lo + RH * CFAR_TILE;                           // rows_whole: T(a) of a guard row
    double* s_ro = s_la + RH * CFAR_TILE;
    double* s_ra = s_ro + RH * CFAR_TILE;
    // counts of Lo | La << 8 | Ro << 16 | Ra << 24; rows_whole: of the outer T | the guard row's T << 16
    uint32_t* s_n = reinterpret_cast<uint32_t*>(s_lo + (rows_whole ? 2 : 4) * RH * CFAR_TILE);
    float* s_v = reinterpret_cast<float*>(s_n + RH * CFAR_TILE);

    // the tile and its halo; what lies outside the map is NaN: in no ring, skipped in every window, no neighbour of an offset
    {
        const int64_t i0 = ti * CFAR_TILE - hd, j0 = (int64_t)tj * CFAR_TILE - hf;
        const bool dfast = (m.sd == 1 || m.sd == -1) && !(m.sf == 1 || m.sf == -1);
        for (int e = tid; e < RH * RW; e += CFAR_T) {
            int r, c;
            if (dfast) c = e / RH, r = e - c * RH;
            else r = e / RW, c = e - r * RW;
            const int64_t i = i0 + r;
            int64_t j = j0 + c;
            if (a.wrap) j += j < 0 ? m.nf : j >= m.nf ? -(int64_t)m.nf : 0;
            float v = __builtin_nanf("");
            if (i >= 0 && i < m.nd && j >= 0 && j < m.nf) v = m.s[i * m.sd + j * m.sf];
            s_v[r * RWp + c] = v;
        }
    }
    __syncthreads();

    // pass 1, along f
    for (int e = tid; e < RH * CFAR_TILE; e += CFAR_T) {
        const int r = e >> 5, c = e & 31;
        const float* row = s_v + r * RWp + c + hf;
        double lo_ = 0.0, li = 0.0, ri = 0.0, ro = 0.0;
        uint32_t nlo = 0, nli = 0, nri = 0, nro = 0;
#pragma unroll 4
        for (int b = -Hf; b < -gf; ++b) cfar_add(row[b], lo_, nlo);
#pragma unroll 2
        for (int b = -gf; b < 0; ++b) cfar_add(row[b], li, nli);
#pragma unroll 2
        for (int b = 1; b <= gf; ++b) cfar_add(row[b], ri, nri);
#pragma unroll 4
        for (int b = gf + 1; b <= Hf; ++b) cfar_add(row[b], ro, nro);
        const double la = lo_ + li, ra = ri + ro;
        if (rows_whole) {
            const float x = row[0];
            const bool f = std::isfinite(x);
            s_lo[e] = (la + ra) + (f ? (double)x : 0.0);
            s_la[e] = lo_ + ro;
            s_n[e] = (nlo + nli + nro + nri + (f ? 1u : 0u)) | (nlo + nro) << 16;
        } else {
            s_lo[e] = lo_, s_la[e] = la, s_ro[e] = ro, s_ra[e] = ra;
            s_n[e] = nlo | (nlo + nli) << 8 | nro << 16 | (nro + nri) << 24;
        }
    }
    __syncthreads();

    // pass 2, along d, and the decision
    const int c = tid & 31;
    const int64_t j = (int64_t)tj * CFAR_TILE + c;
#pragma unroll 1
    for (int k = 0; k < CFAR_CPT; ++k) {
        const int r = (tid >> 5) + k * (CFAR_T / 32);
        const int64_t i = ti * CFAR_TILE + r;
        const int rc = r + hd, cc = c + hf;
        double A = 0.0, B = 0.0, Z = 0.0;
        uint32_t nA = 0, nB = 0, nZ = 0;
        if (rows_whole) {
            const int e0 = rc * CFAR_TILE + c;
#pragma unroll 4
            for (int o = -Hd; o < 0; ++o) {
                const int e = e0 + o * CFAR_TILE;
                const bool outer = o < -gd;
                A += outer ? s_lo[e] : s_la[e];
                nA += outer ? s_n[e] & 0xffff : s_n[e] >> 16;
            }
#pragma unroll 4
            for (int o = 1; o <= Hd; ++o) {
                const int e = e0 + o * CFAR_TILE;
                const bool outer = o > gd;
                B += outer ? s_lo[e] : s_la[e];
                nB += outer ? s_n[e] & 0xffff : s_n[e] >> 16;
            }
            Z = s_la[e0], nZ = s_n[e0] >> 16;
        } else {
#pragma unroll 4
            for (int o = -Hd; o <= Hd; ++o) {
                const int e = (rc + o) * CFAR_TILE + c;
                const uint32_t pk = s_n[e];
                if (o < -gd || o > gd) A += s_la[e], B += s_ra[e], nA += (pk >> 8) & 255, nB += pk >> 24;
                else A += s_lo[e], B += s_ro[e], nA += pk & 255, nB += (pk >> 16) & 255;
            }
        }
        double noise;
        uint32_t n;
        if (a.mode == CAF_CFAR_CA) {
            n = nA + nB + nZ;
            noise = n ? ((A + B) + Z) / (double)n : __builtin_nan("");  // (no ring: the one NaN of the noise map, not the bits of 0 / 0)
        } else {
            n = nA + nB;
            const double mA = nA ? A / (double)nA : __builtin_nan(""), mB = nB ? B / (double)nB : __builtin_nan("");
            if (nA && nB) noise = a.mode == CAF_CFAR_GO ? (mA > mB ? mA : mB) : (mA < mB ? mA : mB);
            else noise = nA ? mA : mB;
        }
        const bool inside = i < m.nd && j < m.nf;
        const float v = s_v[rc * RWp + cc];
        bool det = inside && std::isfinite(v) && (int64_t)n >= a.min_cells && (double)v >= m.floor && (double)v > m.alpha * noise;
        if (det) {  // the first maximum of the window: > what precedes it in (i, j) order, >= what follows
            for (int o = -a.md; o <= a.md && det; ++o) {
                for (int b = -a.mf; b <= a.mf; ++b) {
                    if (o == 0 && b == 0) continue;
                    const float q = s_v[(rc + o) * RWp + cc + b];
                    if (!std::isfinite(q)) continue;
                    int64_t jn = j + b;
                    if (a.wrap) jn += jn < 0 ? m.nf : jn >= m.nf ? -(int64_t)m.nf : 0;
                    const bool before = o < 0 || (o == 0 && jn < j);
                    if (before ? !(v > q) : !(v >= q)) {
                        det = false;
                        break;
                    }
                }
            }
        }
        const unsigned long long ballot = __ballot(det);
        const uint32_t rowmask = (uint32_t)((tid & 32) ? ballot >> 32 : ballot);  // a row of the tile is half a wave
        const int64_t seg = seg_row0 + (int64_t)r * m.ntf;
        if constexpr (!FILL) {
            if (inside && m.noise) m.noise[i * (int64_t)m.nf + j] = (int64_t)n >= a.min_cells ? (float)noise : __builtin_nanf("");
            if (c == 0 && a.cnt) a.cnt[seg] = __popc(rowmask);  // (rows past nd too: every segment is written)
        } else if (det) {
            const int64_t at = cfar_before(a, seg, nseg) - cfar_before(a, m.seg0, nseg) + __popc(rowmask & ((1u << c) - 1u));
            if (at < a.cap) {
                caf_cfar_det d;
                d.i = (int32_t)i, d.j = (int32_t)j;
                d.value = v, d.noise = (float)noise, d.ratio = (float)((double)v / noise);
                d.di = cfar_subcell(s_v[(rc - 1) * RWp + cc], v, s_v[(rc + 1) * RWp + cc]);
                d.dj = cfar_subcell(s_v[rc * RWp + cc - 1], v, s_v[rc * RWp + cc + 1]);
                d.cells = (int32_t)n;
                a.det[(int64_t)lo * a.cap + at] = d;
            }
        }
    }
}

// exclusive scan of the segments' counts within chunks of CFAR_CHUNK, and the chunks' totals
__global__ __launch_bounds__(CFAR_CHUNK) void k_cfar_segscan(const int32_t* __restrict__ cnt, int64_t nseg, int32_t* __restrict__ loc,
                                                             int64_t* __restrict__ ctot) {
    __shared__ int32_t s_wave[CFAR_CHUNK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * CFAR_CHUNK + threadIdx.x;
    const int32_t v = s < nseg ? cnt[s] : 0;
    const int32_t incl = wave_scan_inclusive(v, lane);
    const int32_t off = block_exclusive(incl, v, lane, wave, s_wave);
    if (s < nseg) loc[s] = off;
    if (threadIdx.x == CFAR_CHUNK - 1) ctot[blockIdx.x] = (int64_t)off + v;
}

__global__ __launch_bounds__(CFAR_T) void k_cfar_counts(const CfarArgs a, int64_t* __restrict__ count) {
    const int b = blockIdx.x * CFAR_T + threadIdx.x;
    if (b >= a.B) return;
    const int64_t nseg = a.maps[a.B].seg0;
    count[b] = cfar_before(a, a.maps[b + 1].seg0, nseg) - cfar_before(a, a.maps[b].seg0, nseg);
}

static_assert(cfar_lds(CFAR_HMAX, CFAR_HMAX) <= CFAR_LDS_BUDGET, "the largest window fits the LDS budget");

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// the descriptor's own fields, or a refusal
int32_t cfar_desc_ok(const caf_cfar_desc* d) {
    CAF_REQUIRE(d->B >= 1 && d->B <= CFAR_MAX_B, "caf_cfar_surface: 1 <= B <= 2^20 maps");
    CAF_REQUIRE(d->h_maps != nullptr, "caf_cfar_surface: NULL map array (a host array of B caf_cfar_map)");
    CAF_REQUIRE(d->gd >= 0 && d->gf >= 0 && d->td >= 0 && d->tf >= 0, "caf_cfar_surface: guard and training half widths must not be negative");
    const int64_t Hd = (int64_t)d->gd + d->td, Hf = (int64_t)d->gf + d->tf;
    CAF_REQUIRE(Hd <= CFAR_HMAX && Hf <= CFAR_HMAX, "caf_cfar_surface: Hd = gd + td and Hf = gf + tf are at most 32");
    CAF_REQUIRE(d->td + d->tf >= 1, "caf_cfar_surface: no training cells (td + tf >= 1)");
    CAF_REQUIRE(d->md >= 0 && d->md <= Hd && d->mf >= 0 && d->mf <= Hf, "caf_cfar_surface: 0 <= md <= Hd and 0 <= mf <= Hf");
    CAF_REQUIRE(d->md + d->mf >= 1, "caf_cfar_surface: no local-maximum window (md + mf >= 1)");
    CAF_REQUIRE(d->mode == CAF_CFAR_CA || d->mode == CAF_CFAR_GO || d->mode == CAF_CFAR_SO,
                "caf_cfar_surface: mode must be CAF_CFAR_CA, CAF_CFAR_GO or CAF_CFAR_SO");
    if (d->mode != CAF_CFAR_CA) {
        CAF_REQUIRE(d->split_axis == 0 || d->split_axis == 1, "caf_cfar_surface: split_axis must be 0 (delay) or 1 (frequency)");
        CAF_REQUIRE((d->split_axis == 0 ? Hd : Hf) >= 1, "caf_cfar_surface: GO and SO need a half width of at least 1 on split_axis");
    }
    CAF_REQUIRE(d->wrap_f == 0 || d->wrap_f == 1, "caf_cfar_surface: wrap_f must be 0 or 1");
    CAF_REQUIRE(d->min_cells >= 0, "caf_cfar_surface: min_cells must not be negative");
    CAF_REQUIRE(d->cap >= 0, "caf_cfar_surface: cap must not be negative");
    CAF_REQUIRE(d->cap == 0 || d->d_det != nullptr, "caf_cfar_surface: a cap above 0 needs d_det");
    return CAF_OK;
}

// the maps of the call, or a refusal that names the map; their tiles and segments laid out in `out` (B + 1 entries)
int32_t cfar_maps_ok(const caf_cfar_desc* d, CfarMap* out) {
    const int64_t Hf = (int64_t)d->gf + d->tf;
    int64_t tiles = 0, segs = 0;
    for (int64_t b = 0; b < d->B; ++b) {
        const caf_cfar_map& m = d->h_maps[b];
        const std::string at = " (map " + std::to_string(b) + ")";
        CAF_REQUIRE(m.d_surface != nullptr, "caf_cfar_surface: NULL surface" + at);
        CAF_REQUIRE(m.nd >= 1 && m.nf >= 1, "caf_cfar_surface: a map needs nd >= 1 and nf >= 1" + at);
        CAF_REQUIRE((m.nd == 1 || m.stride_d != 0) && (m.nf == 1 || m.stride_f != 0),
                    "caf_cfar_surface: the stride of an axis with more than one entry must not be 0" + at);
        CAF_REQUIRE(std::isfinite(m.alpha) && m.alpha > 0.0 && std::isfinite(m.floor), "caf_cfar_surface: alpha and floor must be finite, alpha > 0" + at);
        CAF_REQUIRE(!d->wrap_f || 2 * Hf + 1 <= m.nf, "caf_cfar_surface: wrap_f needs 2 Hf + 1 <= nf" + at);
        const int64_t ntd = ((int64_t)m.nd + CFAR_TILE - 1) / CFAR_TILE, ntf = ((int64_t)m.nf + CFAR_TILE - 1) / CFAR_TILE;
        if (out) {
            CfarMap& o = out[b];
            o.s = m.d_surface, o.noise = m.d_noise, o.sd = m.stride_d, o.sf = m.stride_f, o.nd = m.nd, o.nf = m.nf;
            o.ntf = (int32_t)ntf, o.pad = 0, o.tile0 = tiles, o.seg0 = segs, o.alpha = m.alpha, o.floor = m.floor;
        }
        tiles += ntd * ntf;
        segs += ntd * CFAR_TILE * ntf;
        CAF_REQUIRE(tiles <= 0x7fffffff, "caf_cfar_surface: more than 2^31 - 1 tiles of 32 x 32 cells in one call" + at);
    }
    if (out) {
        std::memset(&out[d->B], 0, sizeof(CfarMap));
        out[d->B].tile0 = tiles, out[d->B].seg0 = segs;
    }
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_cfar_geometry(int32_t Hd, int32_t Hf, int32_t* tile_d, int32_t* tile_f, int32_t* threads, int64_t* lds_bytes) {
    CAF_REQUIRE(Hd >= 0 && Hf >= 0 && Hd <= CFAR_HMAX && Hf <= CFAR_HMAX, "caf_cfar_geometry: 0 <= Hd, Hf <= 32");
    if (tile_d) *tile_d = CFAR_TILE;
    if (tile_f) *tile_f = CFAR_TILE;
    if (threads) *threads = CFAR_T;
    if (lds_bytes) *lds_bytes = cfar_lds(Hd, Hf);
    return CAF_OK;
}

int32_t caf_cfar_surface(const caf_cfar_desc* desc) {
    CAF_REQUIRE(desc != nullptr, "caf_cfar_surface: NULL descriptor");
    int rc;
    if ((rc = cfar_desc_ok(desc))) return rc;
    if ((rc = cfar_maps_ok(desc, nullptr))) return rc;
    const int32_t B = desc->B;
    const bool listing = desc->d_count != nullptr || desc->cap > 0;
    bool any_noise = false;
    for (int32_t b = 0; b < B; ++b) any_noise = any_noise || desc->h_maps[b].d_noise != nullptr;
    if (!listing && !any_noise) return CAF_OK;

    CfarArgs a{};
    a.B = B, a.gd = desc->gd, a.gf = desc->gf, a.Hd = desc->gd + desc->td, a.Hf = desc->gf + desc->tf, a.md = desc->md, a.mf = desc->mf;
    a.mode = desc->mode, a.split = desc->mode == CAF_CFAR_CA ? 0 : desc->split_axis, a.wrap = desc->wrap_f, a.min_cells = desc->min_cells;
    a.det = desc->d_det, a.cap = desc->cap;
    const int64_t lds = cfar_lds(a.Hd, a.Hf, a.mode == CAF_CFAR_CA || a.split == 0 ? 2 : 4);

    hipStream_t st = (hipStream_t)desc->stream;
    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    if ((rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_cfar<false>), (size_t)lds))) return rc;
    if ((rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_cfar<true>), (size_t)lds))) return rc;
    const int64_t map_bytes = align16((int64_t)(B + 1) * (int64_t)sizeof(CfarMap));
    Lane* lane = nullptr;
    if ((rc = lane_acquire("caf_cfar_surface", dev, map_bytes, &lane))) return rc;
    CfarMap* h = (CfarMap*)lane->pinned;
    (void)cfar_maps_ok(desc, h);
    const int64_t tiles = h[B].tile0, nseg = h[B].seg0;
    const int64_t nch = (nseg + CFAR_CHUNK - 1) / CFAR_CHUNK;
    const int64_t seg_bytes = listing ? align16(nseg * 4) : 0, chunk_bytes = listing ? align16((nch + 1) * 8) : 0;
    void* d_block = nullptr;
    if ((rc = pool_alloc(&d_block, map_bytes + 2 * seg_bytes + chunk_bytes, st == nullptr))) {
        lane_abandon(lane, nullptr, st);
        return rc;
    }
    a.maps = (const CfarMap*)d_block;
    int64_t* cbase = nullptr;
    int32_t* loc = nullptr;
    if (listing) {
        cbase = (int64_t*)((char*)d_block + map_bytes);
        a.cnt = (int32_t*)((char*)d_block + map_bytes + chunk_bytes);
        loc = (int32_t*)((char*)d_block + map_bytes + chunk_bytes + seg_bytes);
        a.loc = loc, a.cbase = cbase;
    }

    hipError_t e = hipMemcpyAsync(d_block, lane->pinned, (size_t)map_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_cfar<false>, dim3((unsigned)tiles), dim3(CFAR_T), (size_t)lds, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess && listing) {
        hipLaunchKernelGGL(k_cfar_segscan, dim3((unsigned)nch), dim3(CFAR_CHUNK), 0, st, (const int32_t*)a.cnt, nseg, loc, cbase);
        launch_scan_exclusive(cbase, nch, st);
        if (desc->d_count) hipLaunchKernelGGL(k_cfar_counts, dim3(cdiv(B, CFAR_T)), dim3(CFAR_T), 0, st, a, desc->d_count);
        if (desc->cap > 0) hipLaunchKernelGGL(k_cfar<true>, dim3((unsigned)tiles), dim3(CFAR_T), (size_t)lds, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(lane->ev, st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        lane_abandon(lane, d_block, st);
        set_error(std::string("caf_cfar_surface: ") + hipGetErrorString(e));
        return CAF_ERR_HIP;
    }
    lane_in_flight(lane, d_block);
    return CAF_OK;
}
