// chamfer_nd.hip -- the Chamfer distance of D-dimensional clouds, 1 <= D <= 8,
// for MI355X (gfx950, CDNA4): forward with argmin, deterministic backward.
// include/pcm.h has the contract; DESIGN.md section 3.21 has the rationale and
// the numbers.
//
// Forward (one launch, both directions, templated on D).  A workgroup of kNdW
// waves owns kNdQB = 64 * kNdQ consecutive query points; every wave holds ALL of
// them in registers (a lane kNdQ queries x D coordinates).  The candidate cloud
// goes through LDS in SoA tiles of kNdTile points; wave w scans positions
// [w, w + 1) * kNdTile / kNdW of every tile, four candidates a step: one
// ds_read_b128 a coordinate plane, every lane the same address (a broadcast).
// A pair is D subtracts, one multiply, D - 1 fused steps, one compare and two
// selects.  A wave meets its candidates in ascending index order and replaces
// its best on strict '<' from (+inf, 0), so it keeps the lowest index of its
// minimum; a NaN value compares false and never wins (tile padding is NaN).
// The waves' pairs meet in LDS and thread q takes their lexicographic (d, k)
// minimum: ties across waves and tiles go to the lowest index.
//
// Backward (one launch, both clouds, no float atomics).  A lane owns one target
// point.  The other direction's argmin array goes through LDS in tiles of
// kNdBwdTile entries.  A wave takes kNdBwdRuns runs of 64 entries at a time:
// lane l tests entry l of each run against the range of the wave's 64 targets
// and, on a hit, fetches that source point and its graddist from global memory
// (a wave's targets draw about 64 of the sources, so few lanes load, and all
// runs' loads are in flight together).  The hits are then visited in ascending
// order: the source is broadcast from the lane that fetched it (v_readlane) and
// the lane that owns the target adds its term, in the pinned order of
// oracle/pcm_oracle.c (direct term first for cloud 1, last for cloud 2).
//
// No kernel here waits on another workgroup.
#include "pcm_common.h"

namespace {

#ifndef PCM_ND_Q
#define PCM_ND_Q 4
#endif
#ifndef PCM_ND_W
#define PCM_ND_W 8
#endif
constexpr int kNdMaxDim = PCM_CHAMFER_ND_MAX_DIM;
constexpr int kNdMaxN = PCM_CHAMFER_ND_MAX_POINTS;
constexpr int kNdW = PCM_ND_W;           // waves per workgroup, each a share of every tile
constexpr int kNdQ = PCM_ND_Q;           // queries per lane
constexpr int kNdNT = 64 * kNdW;         // threads per workgroup
constexpr int kNdQB = 64 * kNdQ;         // queries per workgroup
constexpr int kNdTile = 1024;            // candidates per LDS tile
constexpr int kNdShare = kNdTile / kNdW; // candidates of a tile a wave scans
constexpr int kNdPad = 4;                // plane stride kNdTile + 4 words: the rows -> SoA scatter spreads over the banks
constexpr int kNdPlane = kNdTile + kNdPad;
constexpr int kNdBwdNT = 256;            // backward: targets (threads) per workgroup
constexpr int kNdBwdTile = 2048;         // backward: argmin entries per LDS tile
static_assert(kNdShare % 4 == 0 && kNdPlane % 4 == 0, "a wave's share is whole 16-byte reads");
static_assert(kNdQB <= kNdNT || kNdQB % kNdNT == 0, "the merge covers the queries in whole passes");
constexpr int kNdBwdRuns = 8;            // backward: runs of 64 entries a wave fetches for at once
static_assert(kNdBwdTile % kNdBwdNT == 0 && kNdBwdTile % (64 * kNdBwdRuns) == 0,
              "backward tile: whole staging passes, whole groups of runs");

// coordinate t of point k of a cloud of np points: rows [np, D] or planes [D, np]
template <int D>
__device__ __forceinline__ size_t nd_at(int planes, int np, int k, int t) {
    return planes ? (size_t)t * np + k : (size_t)k * D + t;
}

template <int D>
__global__ __launch_bounds__(kNdNT) void chamfer_nd_forward_kernel(
    const float *__restrict__ x1, const float *__restrict__ x2, int n, int m, int lay1, int lay2, int nblk1,
    int nblk2, float *__restrict__ dist1, float *__restrict__ dist2, int32_t *__restrict__ idx1,
    int32_t *__restrict__ idx2) {
    constexpr int W = kNdW, Q = kNdQ, T = kNdTile, NT = kNdNT, QB = kNdQB, P = kNdPlane;
    __shared__ __attribute__((aligned(16))) float sC[D * P];
    __shared__ float sD[W][QB];
    __shared__ int sK[W][QB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    int batch, blk;
    bool first;
    pcm_split_bm(pcm_xcd_remap((int)blockIdx.x, (int)gridDim.x), nblk1, nblk2, batch, first, blk);
    const int nq = first ? n : m, nc = first ? m : n;
    const int layq = first ? lay1 : lay2, layc = first ? lay2 : lay1;
    const float *Qp = (first ? x1 : x2) + (size_t)batch * nq * D;
    const float *Cp = (first ? x2 : x1) + (size_t)batch * nc * D;

    // ---- this lane's queries (a missing one scans as zeros and is not stored)
    float q[Q][D];
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) {
        const int qi = blk * QB + qq * 64 + lane;
#pragma unroll
        for (int t = 0; t < D; ++t) q[qq][t] = (qi < nq) ? Qp[nd_at<D>(layq, nq, qi, t)] : 0.f;
    }
    float best[Q];
    int bestk[Q];
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) {
        best[qq] = PCM_INF;
        bestk[qq] = 0;
    }

    const float pad = __builtin_nanf("");
    for (int t0 = 0; t0 < nc; t0 += T) {
        const int cnt = min(T, nc - t0);
        // ---- stage the tile as SoA planes; positions past the cloud's end read as NaN up to the next multiple of 4
        const int cnt4 = (cnt + 3) & ~3;
        if (layc == 0) {
            const float *src = Cp + (size_t)t0 * D;
            for (int f = tid; f < cnt4 * D; f += NT) {
                const int p = f / D, t = f - p * D;
                sC[t * P + p] = (p < cnt) ? src[f] : pad;
            }
        } else {
#pragma unroll
            for (int t = 0; t < D; ++t)
                for (int p = tid; p < cnt4; p += NT) sC[t * P + p] = (p < cnt) ? Cp[(size_t)t * nc + t0 + p] : pad;
        }
        __syncthreads();

        // ---- this wave's share, ascending
        const int lo = wave * kNdShare;
        const int hi = min(cnt4, lo + kNdShare);
        pcm_f4 nv[D];
#pragma unroll
        for (int t = 0; t < D; ++t) nv[t] = *reinterpret_cast<const pcm_f4 *>(&sC[t * P + lo]);
        for (int c = lo; c < hi; c += 4) {
            pcm_f4 v[D];
            // the next step's reads are in flight during this step's arithmetic; past the share's end they
            // fall on candidates of the next share or on the plane's pad words (c + 4 <= kNdTile) and are dropped
#pragma unroll
            for (int t = 0; t < D; ++t) {
                v[t] = nv[t];
                nv[t] = *reinterpret_cast<const pcm_f4 *>(&sC[t * P + c + 4]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = t0 + c + e;
#pragma unroll
                for (int qq = 0; qq < Q; ++qq) {
                    const float c0 = v[0][e] - q[qq][0];
                    float s = c0 * c0;
#pragma unroll
                    for (int t = 1; t < D; ++t) {
                        const float ct = v[t][e] - q[qq][t];
                        s = __builtin_fmaf(ct, ct, s);
                    }
                    const bool take = s < best[qq];  // false for NaN
                    best[qq] = take ? s : best[qq];
                    bestk[qq] = take ? k : bestk[qq];
                }
            }
        }
        __syncthreads();  // the tile is rewritten next
    }

    // ---- the waves' pairs meet: lexicographic (d, k) minimum, waves ascending
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) {
        sD[wave][qq * 64 + lane] = best[qq];
        sK[wave][qq * 64 + lane] = bestk[qq];
    }
    __syncthreads();
    float *dist = (first ? dist1 : dist2) + (size_t)batch * nq;
    int32_t *idx = (first ? idx1 : idx2) + (size_t)batch * nq;
    for (int ql = tid; ql < QB; ql += NT) {
        const int qi = blk * QB + ql;
        float d = sD[0][ql];
        int k = sK[0][ql];
#pragma unroll
        for (int w = 1; w < W; ++w) pcm_lexmin(d, k, sD[w][ql], sK[w][ql]);
        if (qi < nq) {
            dist[qi] = d;
            idx[qi] = k;
        }
    }
}

// One cloud's gradient: `self` (ns points) is the cloud the targets belong to
template <int D>
__global__ __launch_bounds__(kNdBwdNT) void chamfer_nd_backward_kernel(
    const float *__restrict__ x1, const float *__restrict__ x2, int n, int m, int lay1, int lay2, int nblk1,
    int nblk2, const float *__restrict__ gd1, const float *__restrict__ gd2, const int32_t *__restrict__ idx1,
    const int32_t *__restrict__ idx2, float *__restrict__ grad1, float *__restrict__ grad2) {
    constexpr int NT = kNdBwdNT, T = kNdBwdTile;
    __shared__ int sIdx[T];

    const int tid = threadIdx.x;
    const int lane = tid & 63;

    int batch, blk;
    bool first;
    pcm_split_bm(pcm_xcd_remap((int)blockIdx.x, (int)gridDim.x), nblk1, nblk2, batch, first, blk);
    const int ns = first ? n : m, no = first ? m : n;
    const int lays = first ? lay1 : lay2, layo = first ? lay2 : lay1;
    const float *S = (first ? x1 : x2) + (size_t)batch * ns * D;
    const float *O = (first ? x2 : x1) + (size_t)batch * no * D;
    const float *gs = (first ? gd1 : gd2) + (size_t)batch * ns;
    const float *go = (first ? gd2 : gd1) + (size_t)batch * no;
    const int32_t *is = (first ? idx1 : idx2) + (size_t)batch * ns;
    const int32_t *io = (first ? idx2 : idx1) + (size_t)batch * no;
    float *G = (first ? grad1 : grad2) + (size_t)batch * ns * D;

    const int mine = blk * NT + tid;
    const int wbase = mine - lane;  // the wave's first target
    const bool have = mine < ns;

    float p[D], direct[D], acc[D];
#pragma unroll
    for (int t = 0; t < D; ++t) {
        p[t] = 0.f;
        direct[t] = 0.f;
        acc[t] = 0.f;
    }
    if (have) {
        // the contract wants the index inside the other cloud; a wild one is clamped, never followed
        const int k = min(max(is[mine], 0), no - 1);
        const float g = gs[mine] * 2.f;
#pragma unroll
        for (int t = 0; t < D; ++t) {
            p[t] = S[nd_at<D>(lays, ns, mine, t)];
            direct[t] = g * (p[t] - O[nd_at<D>(layo, no, k, t)]);
        }
    }
    if (first) {
#pragma unroll
        for (int t = 0; t < D; ++t) acc[t] = acc[t] + direct[t];
    }

    for (int j0 = 0; j0 < no; j0 += T) {
        const int cnt = min(T, no - j0);
#pragma unroll
        for (int f = tid; f < T; f += NT) sIdx[f] = (f < cnt) ? io[j0 + f] : -1;
        __syncthreads();
        for (int c0 = 0; c0 < cnt; c0 += 64 * kNdBwdRuns) {
            // ---- lane l looks at entry c0 + 64 u + l of each run u; where it names one of this wave's targets the
            // lane fetches that source point: every run's loads are in flight before the first is used
            int v[kNdBwdRuns];
            float gj[kNdBwdRuns], pj[kNdBwdRuns][D];
#pragma unroll
            for (int u = 0; u < kNdBwdRuns; ++u) {
                const int j = c0 + 64 * u + lane;  // < kNdBwdTile: entries past the cloud's end hold -1
                v[u] = sIdx[j];
                const bool hit = (unsigned)(v[u] - wbase) < 64u;
                gj[u] = hit ? go[j0 + j] * 2.f : 0.f;
#pragma unroll
                for (int t = 0; t < D; ++t) pj[u][t] = hit ? O[nd_at<D>(layo, no, j0 + j, t)] : 0.f;
            }
            // ---- the hits ascending (wave-uniform loop): the source is broadcast from the lane that fetched it and
            // the lane that owns the target adds its term
#pragma unroll
            for (int u = 0; u < kNdBwdRuns; ++u) {
                unsigned long long hits = __ballot((unsigned)(v[u] - wbase) < 64u);
                while (hits) {
                    const int src = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    const bool own = __builtin_amdgcn_readlane(v[u], src) == mine;
                    const float g = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gj[u]), src));
#pragma unroll
                    for (int t = 0; t < D; ++t) {
                        const float o = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pj[u][t]), src));
                        const float sum = acc[t] + (-(g * (o - p[t])));
                        acc[t] = own ? sum : acc[t];
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!first) {
#pragma unroll
        for (int t = 0; t < D; ++t) acc[t] = acc[t] + direct[t];
    }
    if (have) {
#pragma unroll
        for (int t = 0; t < D; ++t) G[nd_at<D>(lays, ns, mine, t)] = acc[t];
    }
}

inline int nd_check(int b, int n, int m, int dim, int layout1, int layout2) {
    if (b < 0 || n < 0 || m < 0 || dim < 1) return PCM_ERR_INVALID_ARG;
    if ((layout1 != 0 && layout1 != 1) || (layout2 != 0 && layout2 != 1)) return PCM_ERR_INVALID_ARG;
    if (dim > kNdMaxDim || n > kNdMaxN || m > kNdMaxN) return PCM_ERR_UNSUPPORTED;
    return PCM_OK;
}

template <int D>
void nd_launch_forward(const float *x1, const float *x2, int b, int n, int m, int layout1, int layout2, float *dist1,
                       float *dist2, int32_t *idx1, int32_t *idx2, hipStream_t st) {
    const int nblk1 = (n + kNdQB - 1) / kNdQB, nblk2 = (m + kNdQB - 1) / kNdQB;
    hipLaunchKernelGGL(chamfer_nd_forward_kernel<D>, dim3((unsigned)((long long)b * (nblk1 + nblk2))), dim3(kNdNT), 0,
                       st, x1, x2, n, m, layout1, layout2, nblk1, nblk2, dist1, dist2, idx1, idx2);
}

template <int D>
void nd_launch_backward(const float *x1, const float *x2, int b, int n, int m, int layout1, int layout2,
                        const float *gd1, const float *gd2, const int32_t *idx1, const int32_t *idx2, float *grad1,
                        float *grad2, hipStream_t st) {
    const int nblk1 = (n + kNdBwdNT - 1) / kNdBwdNT, nblk2 = (m + kNdBwdNT - 1) / kNdBwdNT;
    hipLaunchKernelGGL(chamfer_nd_backward_kernel<D>, dim3((unsigned)((long long)b * (nblk1 + nblk2))),
                       dim3(kNdBwdNT), 0, st, x1, x2, n, m, layout1, layout2, nblk1, nblk2, gd1, gd2, idx1, idx2, grad1,
                       grad2);
}

// dim is 1..8 here
#define PCM_ND_DISPATCH(FN, ...)                 \
    switch (dim) {                               \
        case 1: FN<1>(__VA_ARGS__); break;       \
        case 2: FN<2>(__VA_ARGS__); break;       \
        case 3: FN<3>(__VA_ARGS__); break;       \
        case 4: FN<4>(__VA_ARGS__); break;       \
        case 5: FN<5>(__VA_ARGS__); break;       \
        case 6: FN<6>(__VA_ARGS__); break;       \
        case 7: FN<7>(__VA_ARGS__); break;       \
        default: FN<8>(__VA_ARGS__); break;      \
    }

}  // namespace

// Internal (tests, pcm_hip): the forward's tile, queries per workgroup and waves per tile
extern "C" void pcm_tune_chamfer_nd_geometry(int *tile, int *queries, int *waves) {
    if (tile) *tile = kNdTile;
    if (queries) *queries = kNdQB;
    if (waves) *waves = kNdW;
}

extern "C" int pcm_chamfer_nd_forward(const float *x1, const float *x2, int b, int n, int m, int dim, int layout1,
                                      int layout2, float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                                      void *stream) {
    const int bad = nd_check(b, n, m, dim, layout1, layout2);
    if (bad != PCM_OK) return bad;
    if (b == 0 || n == 0 || m == 0) return PCM_OK;  // no query has a candidate: every output stays as it is
    if (!x1 || !x2 || !dist1 || !dist2 || !idx1 || !idx2) return PCM_ERR_INVALID_ARG;
    const long long blocks = (long long)b * ((n + kNdQB - 1) / kNdQB + (m + kNdQB - 1) / kNdQB);
    if (blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    PCM_ND_DISPATCH(nd_launch_forward, x1, x2, b, n, m, layout1, layout2, dist1, dist2, idx1, idx2, st)
    return pcm_launch_status();
}

extern "C" int pcm_chamfer_nd_backward(const float *x1, const float *x2, int b, int n, int m, int dim, int layout1,
                                       int layout2, const float *graddist1, const float *graddist2,
                                       const int32_t *idx1, const int32_t *idx2, float *grad1, float *grad2,
                                       void *stream) {
    const int bad = nd_check(b, n, m, dim, layout1, layout2);
    if (bad != PCM_OK) return bad;
    if (b == 0) return PCM_OK;
    if (n == 0 || m == 0) return PCM_ERR_INVALID_ARG;
    if (!x1 || !x2 || !graddist1 || !graddist2 || !idx1 || !idx2 || !grad1 || !grad2) return PCM_ERR_INVALID_ARG;
    const long long blocks = (long long)b * ((n + kNdBwdNT - 1) / kNdBwdNT + (m + kNdBwdNT - 1) / kNdBwdNT);
    if (blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    PCM_ND_DISPATCH(nd_launch_backward, x1, x2, b, n, m, layout1, layout2, graddist1, graddist2, idx1, idx2, grad1,
                    grad2, st)
    return pcm_launch_status();
}
