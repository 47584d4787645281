// knn.hip -- k nearest neighbours and the repulsion loss for MI355X (gfx950,
// CDNA4).  include/pcm.h has both contracts; DESIGN.md section 3.14 has the
// rationale and the numbers.
//
// pcm_knn.  One wave owns 64 queries, one per lane, and scans the reference
// cloud (all of it, or on a small grid a quarter: "The m split" below) in
// ascending index order through an LDS copy (1024-point
// tiles, x[], y[], z[] planes, four candidates per broadcast ds_read_b128 of
// each plane).  A lane keeps its k best (d, j) pairs sorted in registers: W
// slots (W = 4, 8, 16, 20 or 32, the width at or above k), every slot indexed by a
// compile-time constant (a runtime-indexed register array goes to scratch).
// The W - k slots in front hold -inf, which nothing is below, so the list
// proper is the last k slots and the k-th distance is always slot W - 1.
// Because every lane meets its candidates in ascending j, an equal distance
// never displaces a listed one: the lexicographic (d, j) order needs only the
// strict '<' on d.  NaN and +inf fail that compare against the +inf of an
// empty slot, so they are never listed.
//
// The selection.  An insertion is W compares, W medians of three and 2 W
// selects, and a wave runs it whenever ANY of its 64 lanes accepts a
// candidate -- at k = 20, m = 1024
// nearly every candidate, although one lane accepts only about k (1 +
// ln(m / k)) of them.  So a lane does not insert when it accepts: it appends
// the pair to its own LDS queue (16 entries; one exec-masked ds_write_b64)
// and the wave drains all queues together once any of them is nearly full:
// pass e inserts every lane's e-th entry.  The number of insertion passes is
// then the LARGEST per-lane accept count of the wave, not the size of the
// union.  Entries were screened against the k-th distance of the last drain,
// which is only looser than the current one; the insertion compares again.
// Variant 1 (pcm_tune_knn) is the form this replaced -- ballot, and insert at
// once when any lane accepts -- kept in the tuning build (-DPCM_TUNE,
// libpcm_hip_tune.so) for tools/bench_knn.py to measure against.
//
// pcm_repulsion_loss.  Three launches, all deterministic: the k = 5 self
// search above into the workspace; one workgroup of four waves per 64 points of
// a cloud that adds each point's own four terms and then scans the cloud's 4 n
// (neighbour index or -1 when the term is inactive) entries, staged through
// LDS, for its own index -- each wave a quarter of every tile, in ascending
// order, the four partial sums added in ascending order: no float atomics;
// and one wave that adds the workgroups' loss partials in ascending order.
#include "pcm_common.h"
#include "pcm_internal.h"

namespace {

constexpr int kKnnMaxK = PCM_KNN_MAX_K;
constexpr int kKnnMaxN = PCM_KNN_MAX_POINTS;
constexpr int kKnnTile = 1024;   // reference points per LDS tile (12 KiB)
constexpr int kKnnQueue = 16;    // queue entries per lane (8 KiB a wave)
constexpr int kKnnDrainAt = kKnnQueue - 4;  // four candidates are screened between two checks

struct __attribute__((aligned(8))) KnnEnt {
    float d;
    int j;
};

// (d, j) into the ascending list; j is above every listed index (see above) and d is not NaN
// (the median of three is only pinned for numbers); +inf changes nothing
template <int W>
__device__ __forceinline__ void knn_insert(float (&ld)[W], int (&li)[W], float d, int j) {
    bool hi = d < ld[W - 1];
#pragma unroll
    for (int s = W - 1; s >= 1; --s) {
        const bool lo = d < ld[s - 1];
        ld[s] = __builtin_amdgcn_fmed3f(ld[s - 1], ld[s], d);  // ld[s - 1] <= ld[s]: d clamped between them
        li[s] = lo ? li[s - 1] : (hi ? j : li[s]);
        hi = lo;
    }
    ld[0] = hi ? d : ld[0];
    li[0] = hi ? j : li[0];
}

// pass e inserts every lane's e-th queued pair; a lane past its count offers +inf
template <int W>
__device__ __forceinline__ void knn_drain(float (&ld)[W], int (&li)[W], const KnnEnt *sQ, int &cnt, int lane) {
#pragma unroll 1
    for (int e = 0; e < kKnnQueue; ++e) {
        if (__ballot(e < cnt) == 0ull) break;
        const KnnEnt q = sQ[e * 64 + lane];
        const float d = e < cnt ? q.d : PCM_INF;
        if (__ballot(d < ld[W - 1]) != 0ull) knn_insert<W>(ld, li, d, q.j);
    }
    cnt = 0;
}

// The m split.  One query per lane and one wave per 64 queries is 512 waves at
// B = 32, N = 1024 on a GPU of 1024 SIMDs, and a lone wave cannot hide the LDS
// latency of its own scan (measured: DESIGN.md 3.14).  With S = 4 the workgroup
// is four waves that share the 64 queries; wave w scans the w-th quarter of the
// reference cloud (its own quarter of the LDS tile, its own queues), and the
// four lists are merged pairwise through LDS in two rounds: wave w + step
// stores its list, wave w inserts it entry by entry until no lane takes one
// (the stored list ascends).  The storing wave's indices are all above the
// inserting wave's, so the strict '<' still gives the (d, j) order.
//
// S waves: queries blk * 64 + lane of cloud blockIdx.x / nblk against all m
// reference points of that cloud; QUEUED: the queued selection, else insert at once
template <int W, bool QUEUED, int S>
__global__ __launch_bounds__(64 * S) void knn_kernel(const float *__restrict__ query, const float *__restrict__ ref,
                                                     int n, int m, int planes_q, int planes_r, int k, int nblk,
                                                     float *__restrict__ dist_out, int *__restrict__ idx_out) {
    static_assert(S == 1 || S == 2 || S == 4, "a power of two: the merge is pairwise");
    constexpr int kSub = kKnnTile / S;  // points of the tile that one wave stages and scans
    __shared__ __attribute__((aligned(16))) float sX[kKnnTile];
    __shared__ __attribute__((aligned(16))) float sY[kKnnTile];
    __shared__ __attribute__((aligned(16))) float sZ[kKnnTile];
    __shared__ KnnEnt sQall[QUEUED ? S * kKnnQueue * 64 : 1];
    __shared__ KnnEnt sM[S > 1 ? (S / 2) * W * 64 : 1];

    const int lane = threadIdx.x & 63;
    const int wave = S > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    const int bi = blockIdx.x / nblk;
    const int i = (blockIdx.x - bi * nblk) * 64 + lane;
    const bool real = i < n;
    const PcmLay Lq = pcm_lay(planes_q, n), Lr = pcm_lay(planes_r, m);
    const float *Q = query + (size_t)bi * n * 3;
    const float *R = ref + (size_t)bi * m * 3;
    const float qx = real ? Q[pcm_at(Lq, i, 0)] : 0.f;
    const float qy = real ? Q[pcm_at(Lq, i, 1)] : 0.f;
    const float qz = real ? Q[pcm_at(Lq, i, 2)] : 0.f;
    KnnEnt *sQ = sQall + (QUEUED ? wave * kKnnQueue * 64 : 0);
    float *tX = sX + wave * kSub, *tY = sY + wave * kSub, *tZ = sZ + wave * kSub;

    float ld[W];
    int li[W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
        ld[s] = s < W - k ? -PCM_INF : PCM_INF;
        li[s] = -1;
    }
    int cnt = 0;

    // this wave's candidates: [j0, j1), a multiple of four to a wave but the last
    const int seg = S == 1 ? m : (((m + S - 1) / S + 3) & ~3);
    const int j0 = wave * seg;
    const int j1 = min(m, j0 + seg);  // <= j0: nothing left for this wave
    for (int t0 = 0; t0 < seg; t0 += kSub) {
        __syncthreads();  // the previous tile has been read
        const int cntT = max(0, min(kSub, j1 - (j0 + t0)));
        const int pad4 = (cntT + 3) & ~3;
        // a slot past the candidates holds NaN: its distance is NaN and is never listed
        for (int p = lane; p < pad4; p += 64) {
            const bool in = p < cntT;
            tX[p] = in ? R[pcm_at(Lr, j0 + t0 + p, 0)] : __builtin_nanf("");
            tY[p] = in ? R[pcm_at(Lr, j0 + t0 + p, 1)] : __builtin_nanf("");
            tZ[p] = in ? R[pcm_at(Lr, j0 + t0 + p, 2)] : __builtin_nanf("");
        }
        __syncthreads();
        for (int c = 0; c < pad4; c += 4) {
            const pcm_f4 x4 = *(const pcm_f4 *)&tX[c];
            const pcm_f4 y4 = *(const pcm_f4 *)&tY[c];
            const pcm_f4 z4 = *(const pcm_f4 *)&tZ[c];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float d = pcm_sqd(x4[u] - qx, y4[u] - qy, z4[u] - qz);
                if constexpr (QUEUED) {
                    if (d < ld[W - 1]) {
                        sQ[cnt * 64 + lane] = KnnEnt{d, j0 + t0 + c + u};
                        ++cnt;
                    }
                } else {
                    if (__ballot(d < ld[W - 1]) != 0ull) knn_insert<W>(ld, li, d == d ? d : PCM_INF, j0 + t0 + c + u);
                }
            }
            if constexpr (QUEUED) {
                if (__ballot(cnt > kKnnDrainAt) != 0ull) knn_drain<W>(ld, li, sQ, cnt, lane);
            }
        }
    }
    if constexpr (QUEUED) knn_drain<W>(ld, li, sQ, cnt, lane);

    if constexpr (S > 1) {
#pragma unroll
        for (int step = 1; step < S; step *= 2) {
            KnnEnt *slot = sM + (wave / (2 * step)) * (W * 64);
            if ((wave & (2 * step - 1)) == step) {
#pragma unroll
                for (int s = 0; s < W; ++s) slot[s * 64 + lane] = KnnEnt{ld[s], li[s]};
            }
            __syncthreads();
            if ((wave & (2 * step - 1)) == 0) {
#pragma unroll 1
                for (int e = W - k; e < W; ++e) {
                    const KnnEnt q = slot[e * 64 + lane];
                    if (__ballot(q.d < ld[W - 1]) == 0ull) break;
                    knn_insert<W>(ld, li, q.d, q.j);
                }
            }
            __syncthreads();  // the slots are written again in the next round
        }
        if (wave != 0) return;
    }

    if (real) {
        float *od = dist_out + ((size_t)bi * n + i) * k;
        int *oi = idx_out + ((size_t)bi * n + i) * k;
#pragma unroll
        for (int s = 0; s < W; ++s) {
            const int o = s - (W - k);
            if (o >= 0) {
                od[o] = ld[s];
                oi[o] = li[s];
            }
        }
    }
}

typedef void (*knn_kernel_t)(const float *, const float *, int, int, int, int, int, int, float *, int *);

template <bool QUEUED, int S>
knn_kernel_t knn_instance(int k) {
    if (k <= 4) return knn_kernel<4, QUEUED, S>;
    if (k <= 8) return knn_kernel<8, QUEUED, S>;
    if (k <= 16) return knn_kernel<16, QUEUED, S>;
    if (k <= 20) return knn_kernel<20, QUEUED, S>;  // the reference's KNN(k=20): 20 slots a pass, not 32
    return knn_kernel<32, QUEUED, S>;
}

// Waves per 64 queries.  Below two waves a SIMD of a whole MI355X (1024 SIMDs)
// the reference cloud is split over four waves; from there on one wave scans it
// all and there is no merge (tools/bench_knn.py).
constexpr int kKnnSplitBelow = 2048;
constexpr int kKnnSplit = 4;
inline int knn_default_split(int b, int n) {
    return (long long)b * ((n + 63) / 64) < kKnnSplitBelow ? kKnnSplit : 1;
}

int knn_check(const float *query, const float *ref, int b, int n, int m, int layout_q, int layout_r, int k,
              const float *dist_out, const int32_t *idx_out) {
    if (b < 0 || n < 0 || m < 0 || k < 1) return PCM_ERR_INVALID_ARG;
    if ((layout_q != 0 && layout_q != 1) || (layout_r != 0 && layout_r != 1)) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0 || m == 0) return PCM_ERR_INVALID_ARG;
    if (!query || !ref || !dist_out || !idx_out) return PCM_ERR_INVALID_ARG;
    if (k > kKnnMaxK || n > kKnnMaxN || m > kKnnMaxN) return PCM_ERR_UNSUPPORTED;
    if ((long long)b * ((n + 63) / 64) > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;  // the grid
    return 1;  // a launch is due
}

// variant: 0 = what pcm_knn runs (queued; the split by the size), 1 = insert at once (one wave; compiled
// into the tuning build only), 2 = queued, one wave, 3 = queued, four waves
int knn_launch(int variant, const float *query, const float *ref, int b, int n, int m, int layout_q, int layout_r,
               int k, float *dist_out, int32_t *idx_out, void *stream) {
    if (variant < 0 || variant > 3) return PCM_ERR_INVALID_ARG;
    const int st = knn_check(query, ref, b, n, m, layout_q, layout_r, k, dist_out, idx_out);
    if (st <= 0) return st;
    const int nblk = (n + 63) / 64;
    const int split = variant == 0 ? knn_default_split(b, n) : variant == 3 ? kKnnSplit : 1;
    knn_kernel_t kern = split == 1 ? knn_instance<true, 1>(k) : knn_instance<true, kKnnSplit>(k);
    if (variant == 1) {
#ifdef PCM_TUNE
        kern = knn_instance<false, 1>(k);
#else
        return PCM_ERR_UNSUPPORTED;  // the tuning build only (make tune)
#endif
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)b * nblk)), dim3((unsigned)(64 * split)), 0,
                       (hipStream_t)stream, query, ref, n, m, layout_q, layout_r, k, nblk, dist_out, (int *)idx_out);
    return pcm_launch_status();
}

// ---------------------------------------------------------------------------
// repulsion loss
// ---------------------------------------------------------------------------

constexpr int kRepK = 5;          // slot 0 and the four slots the loss reads
constexpr int kRepPoints = 64;    // points per workgroup of the gradient kernel: one per lane
constexpr int kRepWaves = 4;      // waves that share them: each scans a quarter of every tile's sources
constexpr int kRepThreads = kRepPoints * kRepWaves;
constexpr int kRepTile = 1024;    // source points per LDS tile: 4096 entries and the coordinates (28 KiB)

// points blk * 64 + lane of cloud blockIdx.x / nblk: their four terms, the
// workgroup's loss partial and (gradxyz non-null) their gradient.  Wave 0 adds
// the points' own slots; every wave then scans its quarter of each tile's
// sources for the points' indices, and wave 0 adds the four partial sums.
__global__ __launch_bounds__(kRepThreads) void repulsion_kernel(const float *__restrict__ xyz, int n, int planes,
                                                                float h, float scale, int nblk,
                                                                const float *__restrict__ kd,
                                                                const int *__restrict__ ki,
                                                                double *__restrict__ partial,
                                                                float *__restrict__ gradxyz) {
    constexpr int kQuarter = kRepTile / kRepWaves;
    __shared__ __attribute__((aligned(16))) int sE[4 * kRepTile];
    __shared__ float sPx[kRepTile], sPy[kRepTile], sPz[kRepTile];
    __shared__ float sAcc[3][kRepWaves - 1][kRepPoints];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bi = blockIdx.x / nblk;
    const int i = (blockIdx.x - bi * nblk) * kRepPoints + lane;
    const bool real = i < n;
    const PcmLay L = pcm_lay(planes, n);
    const float *P = xyz + (size_t)bi * n * 3;
    const float *D = kd + (size_t)bi * n * kRepK;
    const int *J = ki + (size_t)bi * n * kRepK;

    const float px = real ? P[pcm_at(L, i, 0)] : 0.f;
    const float py = real ? P[pcm_at(L, i, 1)] : 0.f;
    const float pz = real ? P[pcm_at(L, i, 2)] : 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f;  // sum of (p_other - p_i) over the active terms that touch i
    if (wave == 0) {
        double terms = 0.0;
        if (real) {
            for (int t = 1; t < kRepK; ++t) {
                const float term = h - D[(size_t)i * kRepK + t];
                if (term > 0.f) {
                    terms += (double)term;
                    const int j = min(max(J[(size_t)i * kRepK + t], 0), n - 1);  // in range already: d is finite here
                    ax += P[pcm_at(L, j, 0)] - px;
                    ay += P[pcm_at(L, j, 1)] - py;
                    az += P[pcm_at(L, j, 2)] - pz;
                }
            }
        }
        const double wg = pcm_wave_sum_f64(terms);
        if (lane == 0) partial[blockIdx.x] = wg;
    }
    if (!gradxyz) return;

    const int me = real ? i : -2;  // an inactive entry is -1
    for (int s0 = 0; s0 < n; s0 += kRepTile) {
        __syncthreads();  // the previous tile has been read
        const int cntS = min(kRepTile, n - s0);
        const int pad4 = (cntS + 3) & ~3;  // four sources a step: the sources past the cloud hold -1
        // one source a thread: its four entries and its coordinates (a hit reads them from LDS: a global
        // read there would stall the wave for a round trip at every hit)
        for (int p = tid; p < pad4; p += kRepThreads) {
            const bool in = p < cntS;
            const size_t at = (size_t)(s0 + (in ? p : 0)) * kRepK;
            int4 e;
            e.x = in && (h - D[at + 1]) > 0.f ? J[at + 1] : -1;
            e.y = in && (h - D[at + 2]) > 0.f ? J[at + 2] : -1;
            e.z = in && (h - D[at + 3]) > 0.f ? J[at + 3] : -1;
            e.w = in && (h - D[at + 4]) > 0.f ? J[at + 4] : -1;
            *(int4 *)&sE[4 * p] = e;
            sPx[p] = in ? P[pcm_at(L, s0 + p, 0)] : 0.f;
            sPy[p] = in ? P[pcm_at(L, s0 + p, 1)] : 0.f;
            sPz[p] = in ? P[pcm_at(L, s0 + p, 2)] : 0.f;
        }
        __syncthreads();
        const int sEnd = min(pad4, (wave + 1) * kQuarter);
        for (int s = wave * kQuarter; s < sEnd; s += 4) {
            int4 e4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e4[u] = *(const int4 *)&sE[4 * (s + u)];
            bool hit[4];  // a list holds an index once: at most one slot of a source names this point
#pragma unroll
            for (int u = 0; u < 4; ++u) hit[u] = (e4[u].x == me) | (e4[u].y == me) | (e4[u].z == me) | (e4[u].w == me);
            if (hit[0] | hit[1] | hit[2] | hit[3]) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (hit[u]) {  // ascending source order
                        ax += sPx[s + u] - px;
                        ay += sPy[s + u] - py;
                        az += sPz[s + u] - pz;
                    }
                }
            }
        }
    }
    if (wave > 0) {
        sAcc[0][wave - 1][lane] = ax;
        sAcc[1][wave - 1][lane] = ay;
        sAcc[2][wave - 1][lane] = az;
    }
    __syncthreads();
    if (wave == 0 && real) {
#pragma unroll
        for (int w = 0; w < kRepWaves - 1; ++w) {
            ax += sAcc[0][w][lane];
            ay += sAcc[1][w][lane];
            az += sAcc[2][w][lane];
        }
        float *G = gradxyz + (size_t)bi * n * 3;
        G[pcm_at(L, i, 0)] = scale * ax;
        G[pcm_at(L, i, 1)] = scale * ay;
        G[pcm_at(L, i, 2)] = scale * az;
    }
}

// loss_out[0] = (sum of the partials: ascending within a lane, then the wave's six DPP steps) * inv_count
__global__ __launch_bounds__(64) void repulsion_finish_kernel(const double *__restrict__ partial, int count,
                                                              double inv_count, float *__restrict__ loss_out) {
    double acc = 0.0;
    for (int p = threadIdx.x; p < count; p += 64) acc += partial[p];
    const double total = pcm_wave_sum_f64(acc);
    if (threadIdx.x == 0) loss_out[0] = (float)(total * inv_count);
}

inline int rep_blocks(int n) { return (n + kRepPoints - 1) / kRepPoints; }

// the layout of the workspace: partials (double), then the k = 5 lists' distances and indices
inline size_t rep_partial_bytes(int b, int n) { return (size_t)b * rep_blocks(n) * sizeof(double); }
inline size_t rep_list_elems(int b, int n) { return (size_t)b * n * kRepK; }

}  // namespace

extern "C" int pcm_knn(const float *query, const float *ref, int b, int n, int m, int layout_q, int layout_r, int k,
                       float *dist_out, int32_t *idx_out, void *stream) {
    return knn_launch(0, query, ref, b, n, m, layout_q, layout_r, k, dist_out, idx_out, stream);
}

extern "C" int pcm_tune_knn(int variant, const float *query, const float *ref, int b, int n, int m, int layout_q,
                            int layout_r, int k, float *dist_out, int32_t *idx_out, void *stream) {
    return knn_launch(variant, query, ref, b, n, m, layout_q, layout_r, k, dist_out, idx_out, stream);
}

extern "C" int pcm_tune_knn_default_split(int b, int n) {
    return knn_default_split(b, n);
}

extern "C" size_t pcm_repulsion_workspace_bytes(int b, int n) {
    if (b <= 0 || n <= 0) return 0;
    return rep_partial_bytes(b, n) + rep_list_elems(b, n) * (sizeof(float) + sizeof(int32_t));
}

extern "C" int pcm_repulsion_loss(const float *xyz, int b, int n, int layout, float h, float *loss_out,
                                  float *gradxyz, void *workspace, size_t ws_bytes, void *stream) {
    if (b < 0 || n < 0 || (layout != 0 && layout != 1) || !__builtin_isfinite(h)) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n < kRepK || !xyz || !loss_out) return PCM_ERR_INVALID_ARG;
    if (n > kKnnMaxN) return PCM_ERR_UNSUPPORTED;
    if ((long long)b * ((n + 63) / 64) > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;  // the grid
    if (!workspace || ws_bytes < pcm_repulsion_workspace_bytes(b, n)) return PCM_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return PCM_ERR_INVALID_ARG;

    double *partial = (double *)workspace;
    float *kd = (float *)((char *)workspace + rep_partial_bytes(b, n));
    int32_t *ki = (int32_t *)(kd + rep_list_elems(b, n));
    const int st = knn_launch(0, xyz, xyz, b, n, n, layout, layout, kRepK, kd, ki, stream);
    if (st != PCM_OK) return st;
    const int nblk = rep_blocks(n);
    const double count = 4.0 * (double)b * (double)n;
    hipLaunchKernelGGL(repulsion_kernel, dim3((unsigned)(b * nblk)), dim3(kRepThreads), 0, (hipStream_t)stream, xyz,
                       n, layout, h, (float)(2.0 / count), nblk, (const float *)kd, (const int *)ki, partial,
                       gradxyz);
    hipLaunchKernelGGL(repulsion_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       (const double *)partial, b * nblk, 1.0 / count, loss_out);
    return pcm_launch_status();
}
