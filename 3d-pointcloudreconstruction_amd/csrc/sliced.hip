// sliced.hip -- sliced Wasserstein distance (p = 2, uniform masses) of two
// clouds for MI355X (gfx950, CDNA4): project on l directions, sort each
// projection in the pinned total order, match the two sorted lists as exact 1-D
// transport, and sum the per-slice gradients over the directions without
// atomics.  include/pcm.h has the contract; DESIGN.md section 3.18 has the
// rationale and the numbers.
//
// The sort is a bitonic network over 64-bit composites (key << 32) | index, so
// one unsigned compare is the pinned order and ties fall to the lower index.  A
// thread holds E composites.  Two register layouts cover every stride:
//   blocked  v[e] = element t E + e : strides below E inside the thread, strides
//            E .. 32 E between lanes -- lane distances 1, 2, 4, 8 as DPP operand
//            patterns on the VALU, 16 and 32 by ds_bpermute (the LDS crossbar, no
//            storage);
//   strided  v[e] = element e T + t : strides T and above inside the thread.
// Only a stage whose first stride is 64 E or more goes through LDS, twice: once
// to turn blocked into strided, once to turn back (two barriers a stage: a
// thread rewrites only the slots it read).  With E = 16 a wave sorts 1024
// composites with no LDS storage and no barrier at all: 34 of the 55 steps stay
// inside the thread, 18 are DPP, 3 ds_bpermute.
//
// Launches (a fixed function of the shape):
//   both clouds <= PCM_SLICED_FUSED_MAX_POINTS: sliced_fused (one workgroup a
//     (element, direction), its lower half on cloud 1 and its upper half on
//     cloud 2 at once -- one wave a cloud up to 1024 points, two up to 2048:
//     project, sort, then match out of LDS), then sliced_finish;
//   else: sliced_sort_large (one workgroup of 1024 threads a (element,
//     direction, cloud), E = 16, the sorted composites to the workspace),
//     sliced_match_large, sliced_finish.
// The match writes each slice's value (double) and, for a cloud with a gradient
// pointer, every point's scalar coefficient by ORIGINAL index to the workspace;
// sliced_finish forms sum_li theta_li c in double, ascending li, and the loss.
// No atomics, no waiting between workgroups, nothing kept in the workspace.
#include "pcm_common.h"

namespace {

typedef unsigned long long sl_u64;

constexpr int kSlMaxN = PCM_SLICED_MAX_POINTS;
constexpr int kSlMaxL = PCM_SLICED_MAX_DIRS;
constexpr int kSlFusedMax = PCM_SLICED_FUSED_MAX_POINTS;
constexpr int kSlThreads = 256;        // sliced_fused, sliced_match_large, sliced_finish
constexpr int kSlWaves = kSlThreads / 64;
constexpr int kSlLargeThreads = 1024;  // sliced_sort_large
constexpr int kSlLargeE = 16;          // composites a thread there

constexpr int kSlSmallE = 4;           // sliced_fused: composites a thread of a cloud of at most 256 points
constexpr int kSlFusedE = 16;          // and of a larger one: one wave up to 1024 points, two up to 2048

static_assert(kSlFusedMax == 2 * 64 * kSlFusedE, "the fused kernel sorts a cloud in at most two waves");
static_assert(kSlMaxN == kSlLargeE * kSlLargeThreads, "the large sort holds sixteen composites a thread");

// the pinned key of a projection: ascending unsigned keys are ascending floats, -0.0 before +0.0, NaNs by
// their bits at the two ends
__device__ __forceinline__ unsigned sl_key(float p) {
    const unsigned u = __float_as_uint(p);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sl_value(sl_u64 composite) {
    const unsigned key = (unsigned)(composite >> 32);
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// One dword of the lane (lane ^ LJ).  Inside a row of 16 lanes the xor is a DPP pattern (a VALU operand
// modifier: nothing goes to the LDS crossbar): quad_perm for 1 and 2, row_ror:8 for 8, and for 4 a row_shl:4
// into banks 0 and 2 then a row_shr:4 into banks 1 and 3.  16 and 32 cross rows: ds_bpermute with
// addr = (lane ^ LJ) << 2.
template <int LJ>
__device__ __forceinline__ unsigned sl_dword_from_lane(unsigned v, int addr) {
    const int x = (int)v;
    if constexpr (LJ == 1) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false);  // [1,0,3,2]
    else if constexpr (LJ == 2) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false);  // [2,3,0,1]
    else if constexpr (LJ == 4) {
        const int up = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xf, 0x5, false);  // row_shl:4: lane i reads i + 4
        return (unsigned)__builtin_amdgcn_update_dpp(up, x, 0x114, 0xf, 0xa, false);  // row_shr:4: i reads i - 4
    } else if constexpr (LJ == 8) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x128, 0xf, 0xf, false);  // row_ror:8
    else return (unsigned)__builtin_amdgcn_ds_bpermute(addr, x);
}
template <int LJ>
__device__ __forceinline__ sl_u64 sl_from_lane(sl_u64 v, int addr) {
    const unsigned lo = sl_dword_from_lane<LJ>((unsigned)v, addr);
    const unsigned hi = sl_dword_from_lane<LJ>((unsigned)(v >> 32), addr);
    return ((sl_u64)hi << 32) | lo;
}

__device__ __forceinline__ void sl_cmpswap(sl_u64 &a, sl_u64 &b, bool up) {
    const sl_u64 x = a, y = b;
    const bool sw = (x > y) == up;
    a = sw ? y : x;
    b = sw ? x : y;
}

// One step between lanes of the blocked layout: every element against the same element of lane ^ LJ
template <int E, int LJ, int CAP>
__device__ __forceinline__ void sl_lane_step(sl_u64 (&v)[CAP], int t, int k) {
    const int addr = (((int)threadIdx.x & 63) ^ LJ) << 2;
    const bool up = ((t * E) & k) == 0;  // k >= 2 j >= 2 E: the same for the thread's E elements
    const bool keepmin = ((t & LJ) == 0) == up;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const sl_u64 o = sl_from_lane<LJ>(v[e], addr);
        v[e] = ((o < v[e]) == keepmin) ? o : v[e];
    }
}

// Blocked layout (v[e] = element t E + e): the steps j = jfirst, jfirst / 2, .. 1 of stage k; jfirst < 64 E.
// Every lane of the wave takes part.
template <int E, int CAP>
__device__ __forceinline__ void sl_blocked(sl_u64 (&v)[CAP], int t, int k, int jfirst) {
    for (int j = jfirst; j >= E; j >>= 1) {  // between lanes
        switch (j / E) {
            case 1: sl_lane_step<E, 1>(v, t, k); break;
            case 2: sl_lane_step<E, 2>(v, t, k); break;
            case 4: sl_lane_step<E, 4>(v, t, k); break;
            case 8: sl_lane_step<E, 8>(v, t, k); break;
            case 16: sl_lane_step<E, 16>(v, t, k); break;
            default: sl_lane_step<E, 32>(v, t, k); break;
        }
    }
#pragma unroll
    for (int j = E / 2; j >= 1; j >>= 1) {  // inside the thread
        if (j <= jfirst) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if ((e & j) == 0) sl_cmpswap(v[e], v[e | j], ((t * E + e) & k) == 0);
            }
        }
    }
}

// Strided layout (v[e] = element e T + t): the steps j = jfirst, .. T of stage k, all inside the thread
template <int E, int CAP>
__device__ __forceinline__ void sl_strided(sl_u64 (&v)[CAP], int T, int k, int jfirst) {
#pragma unroll
    for (int je = E / 2; je >= 1; je >>= 1) {
        if (je * T <= jfirst) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if ((e & je) == 0) sl_cmpswap(v[e], v[e | je], ((e * T) & k) == 0);  // k >= 2 T
            }
        }
    }
}

// Sorts the P = E T composites held blocked by threads 0 .. T - 1 (T a power of two, 64 <= T <= 64 E) and
// leaves them blocked: element t E + e has rank t E + e.  s: P slots of LDS, used only when P > 64 E.  The
// whole workgroup calls this; threads from T on only join the barriers.
template <int E>
__device__ __forceinline__ void sl_sort(sl_u64 (&v)[E], sl_u64 *s, int t, int T) {
    const bool act = t < T;
    const int P = E * T;
    for (int k = 2; k <= P; k <<= 1) {
        int j = k >> 1;
        if (j >= 64 * E) {  // uniform over the workgroup
            if (act) {
#pragma unroll
                for (int e = 0; e < E; ++e) s[t * E + e] = v[e];
            }
            __syncthreads();
            if (act) {
#pragma unroll
                for (int e = 0; e < E; ++e) v[e] = s[e * T + t];
                sl_strided<E>(v, T, k, j);
#pragma unroll
                for (int e = 0; e < E; ++e) s[e * T + t] = v[e];  // the slots this thread alone read
            }
            __syncthreads();
            if (act) {
#pragma unroll
                for (int e = 0; e < E; ++e) v[e] = s[t * E + e];  // which it alone rewrites next time
            }
            j = T >> 1;
        }
        if (act) sl_blocked<E>(v, t, k, j);
    }
}

// The composites of the cloud's points t, t + T, .. t + (E - 1) T on direction (tx, ty, tz) -- which slot a
// point starts in does not matter to a sort, and consecutive lanes read consecutive points; from cnt on the
// padding: the largest key and an index no point has, so it sorts after a positive NaN of all-ones payload
template <int E, int CAP>
__device__ __forceinline__ void sl_load(sl_u64 (&v)[CAP], const float *__restrict__ P, PcmLay L, int cnt, int t,
                                        int T, float tx, float ty, float tz) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * T + t;
        unsigned key = 0xFFFFFFFFu;
        if (i < cnt) {
            const float x = P[pcm_at(L, i, 0)], y = P[pcm_at(L, i, 1)], z = P[pcm_at(L, i, 2)];
            key = sl_key(__builtin_fmaf(tz, z, __builtin_fmaf(ty, y, tx * x)));
        }
        v[e] = ((sl_u64)key << 32) | (unsigned)i;
    }
}

// Project and sort one cloud with T = padded / E threads.  out: where rank r's composite goes for r < lim
// (LDS with lim = padded in the fused kernel, the workspace with lim = cnt in the large one); order: NULL
// or the cloud's [cnt] row of order*_out.
template <int E>
__device__ __forceinline__ void sl_sort_cloud(const float *__restrict__ P, PcmLay L, int cnt, int padded, float tx,
                                              float ty, float tz, sl_u64 *s, sl_u64 *out, int lim,
                                              int *__restrict__ order) {
    const int t = threadIdx.x, T = padded / E;
    sl_u64 v[E];
    if (t < T) sl_load<E>(v, P, L, cnt, t, T, tx, ty, tz);
    sl_sort<E>(v, s, t, T);
    if (t < T) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int r = t * E + e;
            if (r < lim) out[r] = v[e];
            if (order && r < cnt) order[r] = (int)(unsigned)v[e];
        }
    }
}

// Thread's share of the exact transport between the sorted lists A (na points) and B (nb): for its ranks
// r = threadIdx.x, + blockDim.x, .. the overlapping ranks s ascending, in double.  Returns its part of
// sum w (a - b)^2; coef (NULL, or the [na] row by ORIGINAL index): scale * sum_s w (a_r - b_s), rounded once.
template <bool SLICE>
__device__ __forceinline__ double sl_match(const sl_u64 *A, int na, const sl_u64 *B, int nb, double scale,
                                           float *__restrict__ coef) {
    double part = 0.0;
    const bool same = na == nb;  // then rank r meets rank r alone, with weight na: the same sums without the divisions
    for (int r = threadIdx.x; r < na; r += (int)blockDim.x) {
        const sl_u64 ca = A[r];
        const double a = (double)sl_value(ca);
        const int lo = same ? r : (r * nb) / na;                    // (r + 1) nb <= 2^28
        const int hi = same ? r : ((r + 1) * nb + na - 1) / na - 1;  // <= nb - 1
        double cs = 0.0, q = 0.0;
        for (int s = lo; s <= hi; ++s) {
            const double d = a - (double)sl_value(B[s]);
            const int w = min((r + 1) * nb, (s + 1) * na) - max(r * nb, s * na);
            const double wd = (double)w * d;
            cs += wd;
            if constexpr (SLICE) q += wd * d;
        }
        part += q;
        if (coef) coef[(unsigned)ca] = (float)(scale * cs);
    }
    return part;
}

// The (element, direction) pair `pair` from its sorted lists: the slice and the coefficient rows.  sRed:
// kSlWaves doubles of LDS.  Full workgroup (of at most kSlThreads), uniform control flow.
__device__ __forceinline__ void sl_match_block(const sl_u64 *A, int n, const sl_u64 *B, int m, size_t pair,
                                               double *sRed, double *__restrict__ slices,
                                               float *__restrict__ slices_out, float *__restrict__ coef1,
                                               float *__restrict__ coef2) {
    const double nm = (double)n * (double)m, scale = 2.0 / nm;
    const double part = sl_match<true>(A, n, B, m, scale, coef1 ? coef1 + pair * (size_t)n : nullptr);
    if (coef2) sl_match<false>(B, m, A, n, scale, coef2 + pair * (size_t)m);
    const double wsum = pcm_wave_sum_f64(part);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += sRed[w];
        const double slice = total / nm;
        slices[pair] = slice;
        if (slices_out) slices_out[pair] = (float)slice;
    }
}

// One workgroup an (element, direction): LDS holds the pad1 + pad2 sorted composites, then kSlWaves doubles
__global__ __launch_bounds__(kSlThreads) void sliced_fused(const float *__restrict__ xyz1,
                                                           const float *__restrict__ xyz2, int n, int m, int planes1,
                                                           int planes2, const float *__restrict__ dirs, int l,
                                                           int pad1, int pad2, double *__restrict__ slices,
                                                           float *__restrict__ slices_out, float *__restrict__ coef1,
                                                           float *__restrict__ coef2, int *__restrict__ order1,
                                                           int *__restrict__ order2) {
    extern __shared__ __attribute__((aligned(16))) sl_u64 sl_lds[];
    const int id = pcm_xcd_remap(blockIdx.x, gridDim.x);
    const int bi = id / l, li = id - bi * l;
    const size_t pair = (size_t)id;
    const float tx = dirs[3 * li], ty = dirs[3 * li + 1], tz = dirs[3 * li + 2];
    // the lower half of the workgroup sorts cloud 1, the upper half cloud 2, at once
    const int H = (int)blockDim.x >> 1;
    const int c = (int)threadIdx.x >= H ? 1 : 0, t = (int)threadIdx.x - c * H;
    const int cnt = c ? m : n, padded = c ? pad2 : pad1;
    const float *P = (c ? xyz2 : xyz1) + (size_t)bi * cnt * 3;
    const PcmLay L = pcm_lay(c ? planes2 : planes1, cnt);
    sl_u64 *s = sl_lds + (c ? pad1 : 0);
    int *order = c ? order2 : order1;
    if (order) order += pair * (size_t)cnt;
    const bool small = padded <= 64 * kSlSmallE;  // E = 4 in one wave; else E = 16 in one wave or two
    const int T = small ? 64 : padded / kSlFusedE;
    sl_u64 v[kSlFusedE];
    // every stage up to 1024 stays in registers and lanes: no barrier, the waves run on their own
    if (t < T) {
        if (small) {
            sl_load<kSlSmallE>(v, P, L, cnt, t, T, tx, ty, tz);
            for (int k = 2; k <= 64 * kSlSmallE; k <<= 1) sl_blocked<kSlSmallE>(v, t, k, k >> 1);
        } else {
            sl_load<kSlFusedE>(v, P, L, cnt, t, T, tx, ty, tz);
            for (int k = 2; k <= 64 * kSlFusedE; k <<= 1) sl_blocked<kSlFusedE>(v, t, k, k >> 1);
        }
    }
    // the stage 2048 of a cloud above 1024 points (E = 16, T = 128 = H): its stride 1024 through LDS.  The
    // condition is uniform over the workgroup; a half whose cloud is smaller only joins the barriers.
    if (pad1 > 64 * kSlFusedE || pad2 > 64 * kSlFusedE) {
        const bool mine = padded > 64 * kSlFusedE;
        if (mine) {
#pragma unroll
            for (int e = 0; e < kSlFusedE; ++e) s[t * kSlFusedE + e] = v[e];
        }
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int e = 0; e < kSlFusedE; ++e) v[e] = s[e * T + t];
            sl_strided<kSlFusedE>(v, T, padded, padded >> 1);
#pragma unroll
            for (int e = 0; e < kSlFusedE; ++e) s[e * T + t] = v[e];  // the slots this thread alone read
        }
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int e = 0; e < kSlFusedE; ++e) v[e] = s[t * kSlFusedE + e];
        }
        __syncthreads();  // every slot has been read before the sorted list is published over it below
        if (mine) sl_blocked<kSlFusedE>(v, t, padded, T >> 1);
    }
    // Rank r = t E + e sits in v[e].  It is published at slot (r mod E) T + r div E, so that consecutive lanes
    // write consecutive slots; the other half reads its partners from there.
    const int E = small ? kSlSmallE : kSlFusedE;
    if (t < T) {
#pragma unroll
        for (int e = 0; e < kSlFusedE; ++e) {
            if (e < E) {
                s[e * T + t] = v[e];
                const int r = t * E + e;
                if (order && r < cnt) order[r] = (int)(unsigned)v[e];
            }
        }
    }
    __syncthreads();
    // The match: each half takes its own cloud's ranks out of its registers against the other cloud's list --
    // half 0 gives the slice and cloud 1's coefficients, half 1 cloud 2's coefficients.
    const int cntO = c ? n : m, padO = c ? pad1 : pad2;
    const sl_u64 *sO = sl_lds + (c ? 0 : pad1);
    const bool smallO = padO <= 64 * kSlSmallE;
    const int logEO = smallO ? 2 : 4, TO = smallO ? 64 : padO / kSlFusedE;
    const double nm = (double)n * (double)m, scale = 2.0 / nm;
    float *coef = c ? coef2 : coef1;
    if (coef) coef += pair * (size_t)cnt;
    const bool same = n == m;  // then rank r meets rank r alone, with weight n: the same sums without the divisions
    double part = 0.0;
    if (t < T && (c == 0 || coef)) {
#pragma unroll
        for (int e = 0; e < kSlFusedE; ++e) {
            const int r = t * E + e;
            if (e < E && r < cnt) {
                const double a = (double)sl_value(v[e]);
                const int lo = same ? r : (r * cntO) / cnt;                      // (r + 1) cntO <= 2^22
                const int hi = same ? r : ((r + 1) * cntO + cnt - 1) / cnt - 1;  // <= cntO - 1
                double cs = 0.0, q = 0.0;
                for (int so = lo; so <= hi; ++so) {
                    const sl_u64 co = sO[(so & ((1 << logEO) - 1)) * TO + (so >> logEO)];
                    const double d = a - (double)sl_value(co);
                    const int w = min((r + 1) * cntO, (so + 1) * cnt) - max(r * cntO, so * cnt);
                    const double wd = (double)w * d;
                    cs += wd;
                    q += wd * d;
                }
                part += q;
                if (coef) coef[(unsigned)v[e]] = (float)(scale * cs);
            }
        }
    }
    // the slice from half 0: a thread's ranks ascending, a wave by the six DPP steps, the waves ascending
    double *sRed = (double *)(sl_lds + pad1 + pad2);
    const double wsum = pcm_wave_sum_f64(part);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < (H >> 6); ++w) total += sRed[w];
        const double slice = total / nm;
        slices[pair] = slice;
        if (slices_out) slices_out[pair] = (float)slice;
    }
}

// One workgroup an (element, direction, cloud): LDS holds max(pad1, pad2) composites
__global__ __launch_bounds__(kSlLargeThreads) void sliced_sort_large(const float *__restrict__ xyz1,
                                                                     const float *__restrict__ xyz2, int n, int m,
                                                                     int planes1, int planes2,
                                                                     const float *__restrict__ dirs, int l, int pad1,
                                                                     int pad2, sl_u64 *__restrict__ sorted1,
                                                                     sl_u64 *__restrict__ sorted2,
                                                                     int *__restrict__ order1,
                                                                     int *__restrict__ order2) {
    extern __shared__ __attribute__((aligned(16))) sl_u64 sl_lds[];
    const int id = pcm_xcd_remap(blockIdx.x, gridDim.x);
    const int c = id & 1, pr = id >> 1;
    const int bi = pr / l, li = pr - bi * l;
    const size_t pair = (size_t)pr;
    const float tx = dirs[3 * li], ty = dirs[3 * li + 1], tz = dirs[3 * li + 2];
    const int cnt = c ? m : n, padded = c ? pad2 : pad1;
    const float *P = (c ? xyz2 : xyz1) + (size_t)bi * cnt * 3;
    const PcmLay L = pcm_lay(c ? planes2 : planes1, cnt);
    sl_u64 *out = (c ? sorted2 : sorted1) + pair * (size_t)cnt;
    int *order = c ? order2 : order1;
    if (order) order += pair * (size_t)cnt;
    sl_sort_cloud<kSlLargeE>(P, L, cnt, padded, tx, ty, tz, sl_lds, out, cnt, order);
}

__global__ __launch_bounds__(kSlThreads) void sliced_match_large(const sl_u64 *__restrict__ sorted1,
                                                                 const sl_u64 *__restrict__ sorted2, int n, int m,
                                                                 double *__restrict__ slices,
                                                                 float *__restrict__ slices_out,
                                                                 float *__restrict__ coef1,
                                                                 float *__restrict__ coef2) {
    __shared__ double sRed[kSlWaves];
    const size_t pair = (size_t)pcm_xcd_remap(blockIdx.x, gridDim.x);
    sl_match_block(sorted1 + pair * (size_t)n, n, sorted2 + pair * (size_t)m, m, pair, sRed, slices, slices_out,
                   coef1, coef2);
}

// Element bid / per: its nblk1 blocks of cloud 1's gradient (0 without the pointer), the nblk2 of cloud 2's,
// then the loss block.  A gradient block owns 64 points, a lane one point: wave w adds theta_li c[li][i] in
// double over its quarter of the directions, li in [w q, min(l, (w + 1) q)) with q = ceil(l / 4), ascending;
// wave 0 adds the quarters ascending, divides by l and rounds once.  The loss block: thread t adds slices t, t + 256, .. ascending, every wave
// its 64 threads by the six DPP steps, thread 0 the four waves' sums ascending; divided by l, rounded once.
__global__ __launch_bounds__(kSlThreads) void sliced_finish(const float *__restrict__ dirs, int l, int n, int m,
                                                            int planes1, int planes2, int nblk1, int nblk2,
                                                            const double *__restrict__ slices,
                                                            const float *__restrict__ coef1,
                                                            const float *__restrict__ coef2,
                                                            float *__restrict__ loss_out,
                                                            float *__restrict__ gradxyz1,
                                                            float *__restrict__ gradxyz2) {
    __shared__ float sDir[3 * kSlMaxL];
    __shared__ double sRed[kSlWaves];
    __shared__ double sPart[(kSlWaves - 1) * 3 * 64];
    const int per = nblk1 + nblk2 + 1;
    const int bi = blockIdx.x / per, r = blockIdx.x - bi * per;
    if (r == per - 1) {
        const double *S = slices + (size_t)bi * l;
        double acc = 0.0;
        for (int li = threadIdx.x; li < l; li += kSlThreads) acc += S[li];
        const double wsum = pcm_wave_sum_f64(acc);
        if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = wsum;
        __syncthreads();
        if (threadIdx.x == 0) {
            double total = 0.0;
            for (int w = 0; w < kSlWaves; ++w) total += sRed[w];
            loss_out[bi] = (float)(total / (double)l);
        }
        return;
    }
    for (int k = threadIdx.x; k < 3 * l; k += kSlThreads) sDir[k] = dirs[k];
    __syncthreads();
    const bool first = r < nblk1;
    const int cnt = first ? n : m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (first ? r : r - nblk1) * 64 + lane;
    const int at = i < cnt ? i : cnt - 1;  // a lane past the cloud adds the last point's terms and writes nothing
    const float *C = (first ? coef1 : coef2) + (size_t)bi * l * cnt + at;
    const int q = (l + kSlWaves - 1) / kSlWaves, beg = wave * q, end = min(l, beg + q);
    double ax = 0.0, ay = 0.0, az = 0.0;
#pragma unroll 8
    for (int li = beg; li < end; ++li) {
        const double c = (double)C[(size_t)li * cnt];
        ax += (double)sDir[3 * li] * c;
        ay += (double)sDir[3 * li + 1] * c;
        az += (double)sDir[3 * li + 2] * c;
    }
    if (wave > 0) {
        sPart[((wave - 1) * 3 + 0) * 64 + lane] = ax;
        sPart[((wave - 1) * 3 + 1) * 64 + lane] = ay;
        sPart[((wave - 1) * 3 + 2) * 64 + lane] = az;
    }
    __syncthreads();
    if (wave > 0 || i >= cnt) return;
    for (int w = 0; w < kSlWaves - 1; ++w) {  // the quarters ascending
        ax += sPart[(w * 3 + 0) * 64 + lane];
        ay += sPart[(w * 3 + 1) * 64 + lane];
        az += sPart[(w * 3 + 2) * 64 + lane];
    }
    float *G = (first ? gradxyz1 : gradxyz2) + (size_t)bi * cnt * 3;
    const PcmLay L = pcm_lay(first ? planes1 : planes2, cnt);
    G[pcm_at(L, i, 0)] = (float)(ax / (double)l);
    G[pcm_at(L, i, 1)] = (float)(ay / (double)l);
    G[pcm_at(L, i, 2)] = (float)(az / (double)l);
}

inline int sl_pow2(int n, int least) {
    int p = least;
    while (p < n) p <<= 1;
    return p;
}
// slots a cloud takes in sliced_fused: 256 (one wave of E = 4), 1024 (one wave of E = 16) or 2048 (two)
inline int sl_fused_pad(int n) {
    return n <= 64 * kSlSmallE ? 64 * kSlSmallE : n <= 64 * kSlFusedE ? 64 * kSlFusedE : kSlFusedMax;
}
inline bool sl_large(int n, int m) { return n > kSlFusedMax || m > kSlFusedMax; }

}  // namespace

// workspace: [b l] doubles (the slices); when a cloud is above the fused size the sorted composites
// [b l n] and [b l m] (8 bytes each); the coefficient rows [b l n] and [b l m] floats
extern "C" size_t pcm_sliced_workspace_bytes(int b, int n, int m, int l) {
    if (b <= 0 || n <= 0 || m <= 0 || l <= 0) return 0;
    const size_t pairs = (size_t)b * (size_t)l, pts = (size_t)n + (size_t)m;
    return pairs * sizeof(double) + (sl_large(n, m) ? pairs * pts * sizeof(sl_u64) : 0) + pairs * pts * sizeof(float);
}

extern "C" int pcm_sliced_wasserstein_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1,
                                           int layout2, const float *dirs, int l, float *loss_out, float *slices_out,
                                           float *gradxyz1, float *gradxyz2, int *order1_out, int *order2_out,
                                           void *workspace, size_t workspace_bytes, void *stream) {
    if (b < 0 || n < 0 || m < 0) return PCM_ERR_INVALID_ARG;
    if ((layout1 != 0 && layout1 != 1) || (layout2 != 0 && layout2 != 1)) return PCM_ERR_INVALID_ARG;
    if (l <= 0) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0 || m == 0 || !xyz1 || !xyz2 || !dirs || !loss_out) return PCM_ERR_INVALID_ARG;
    if (n > kSlMaxN || m > kSlMaxN || l > kSlMaxL) return PCM_ERR_UNSUPPORTED;
    if ((long long)b * l * 2 > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;  // the grids
    const int nblk1 = gradxyz1 ? (n + 63) / 64 : 0;  // sliced_finish: 64 points a workgroup
    const int nblk2 = gradxyz2 ? (m + 63) / 64 : 0;
    if ((long long)b * (nblk1 + nblk2 + 1) > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < pcm_sliced_workspace_bytes(b, n, m, l)) return PCM_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return PCM_ERR_INVALID_ARG;

    const size_t pairs = (size_t)b * (size_t)l;
    const bool large = sl_large(n, m);
    double *slices = (double *)workspace;
    sl_u64 *sorted1 = (sl_u64 *)(slices + pairs), *sorted2 = sorted1 + (large ? pairs * (size_t)n : 0);
    float *coef1 = (float *)(sorted2 + (large ? pairs * (size_t)m : 0)), *coef2 = coef1 + pairs * (size_t)n;
    float *c1 = gradxyz1 ? coef1 : nullptr, *c2 = gradxyz2 ? coef2 : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (!large) {
        const int pad1 = sl_fused_pad(n), pad2 = sl_fused_pad(m);
        const size_t lds = ((size_t)pad1 + pad2) * sizeof(sl_u64) + kSlWaves * sizeof(double);
        const int threads = (pad1 > 64 * kSlFusedE || pad2 > 64 * kSlFusedE) ? kSlThreads : kSlThreads / 2;
        hipLaunchKernelGGL(sliced_fused, dim3((unsigned)pairs), dim3(threads), lds, st, xyz1, xyz2, n, m, layout1,
                           layout2, dirs, l, pad1, pad2, slices, slices_out, c1, c2, order1_out, order2_out);
    } else {
        const int pad1 = sl_pow2(n, 64 * kSlLargeE), pad2 = sl_pow2(m, 64 * kSlLargeE);  // at least one wave
        const size_t lds = (size_t)(pad1 > pad2 ? pad1 : pad2) * sizeof(sl_u64);
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute((const void *)sliced_sort_large, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            return PCM_ERR_LAUNCH;
        hipLaunchKernelGGL(sliced_sort_large, dim3((unsigned)(2 * pairs)), dim3(kSlLargeThreads), lds, st, xyz1, xyz2,
                           n, m, layout1, layout2, dirs, l, pad1, pad2, sorted1, sorted2, order1_out, order2_out);
        hipLaunchKernelGGL(sliced_match_large, dim3((unsigned)pairs), dim3(kSlThreads), 0, st,
                           (const sl_u64 *)sorted1, (const sl_u64 *)sorted2, n, m, slices, slices_out, c1, c2);
    }
    hipLaunchKernelGGL(sliced_finish, dim3((unsigned)(b * (nblk1 + nblk2 + 1))), dim3(kSlThreads), 0, st, dirs, l, n,
                       m, layout1, layout2, nblk1, nblk2, (const double *)slices, (const float *)c1,
                       (const float *)c2, loss_out, gradxyz1, gradxyz2);
    return pcm_launch_status();
}
