// kernel_loss.hip -- kernel-norm (MMD) losses of two clouds for MI355X (gfx950,
// CDNA4): Gaussian, Laplacian and energy distance, with both gradients from the
// same scan.  include/pcm.h has the contract; DESIGN.md section 3.16 has the
// rationale and the numbers.  The formulas are geomloss's published ones;
// geomloss is not installed here, so they are NOT verified against that
// package (include/pcm.h says the same).
//
// Two launches, both deterministic:
//   1. kernel_loss_scan.  A workgroup of eight waves owns kKlRows = 128 points
//      ("rows") of ONE cloud of one element, two to a lane in registers, so two
//      independent exponentials are in flight per column.  The columns -- first
//      the rows' own cloud, then the other one -- go through an LDS tile of
//      kKlTile = 1024 points packed (x, y, z, -): one ds_read_b128 at a
//      wave-uniform address (a broadcast) feeds both rows of every lane.  Wave w
//      takes the w-th eighth of every tile, so the scan always runs eight waves
//      a workgroup whatever the grid (32 clouds of 1024 + 1024 points: 512
//      workgroups, four waves a SIMD) and the order of every sum depends on
//      (n, m) alone.  Per row a lane keeps S = sum k and V = sum g (p - q) for
//      the own and the other cloud: eight float32 accumulators, two without
//      gradients.  The waves' sums meet in LDS (the tile's storage) and wave 0
//      adds them in ascending wave order, writes the row's two S to the workspace
//      and its gradient to gradxyz.  A cloud without a gradient pointer runs
//      the two-accumulator form: the same S bits.
//   2. kernel_loss_finish: one workgroup an element adds the rows' terms in
//      double in a fixed order and rounds once.
// No atomics, no waiting between workgroups, nothing kept in the workspace.
#include "pcm_common.h"

namespace {

constexpr int kKlMaxN = PCM_KERNEL_LOSS_MAX_POINTS;
constexpr int kKlWaves = 8;                  // waves per workgroup: each an eighth of every tile
constexpr int kKlThreads = 64 * kKlWaves;
constexpr int kKlPerLane = 2;                // rows per lane
constexpr int kKlRows = 64 * kKlPerLane;     // rows per workgroup
constexpr int kKlTile = 1024;                // column points per LDS tile (16 KiB)
constexpr int kKlShare = kKlTile / kKlWaves;
constexpr int kKlFinishThreads = 256;

// float4 slots of the workgroup's LDS: the tile, or the sums of waves 1.. that take its place at the end
// (eight accumulators a row: 28 KiB), whichever is more
constexpr int kKlMergeSlots = (kKlWaves - 1) * 8 * kKlRows / 4;
constexpr int kKlShared = kKlMergeSlots > kKlTile ? kKlMergeSlots : kKlTile;

// k and g of one pair from its pinned squared distance; c: the exponent's scale
template <int K>
__device__ __forceinline__ void kl_pair(float d2, float c, float &k, float &g) {
    if constexpr (K == PCM_KERNEL_GAUSSIAN) {
        k = __builtin_amdgcn_exp2f(d2 * c);
        g = k;
    } else if constexpr (K == PCM_KERNEL_LAPLACIAN) {
        const float r = __builtin_sqrtf(d2);  // the root and the quotient correctly rounded
        k = __builtin_amdgcn_exp2f(r * c);
        g = r > 0.f ? k / r : 0.f;            // a coincident pair adds nothing: the subgradient
    } else {
        const float r = __builtin_sqrtf(d2);
        k = -r;
        g = r > 0.f ? 1.0f / r : 0.f;
    }
}

// The rows' sums against the cloud Q of `cnt` points: this wave's share of every tile, ascending.
// Full workgroup, uniform control flow.
template <int K, bool GRAD>
__device__ __forceinline__ void kl_scan(const float *__restrict__ Q, PcmLay L, int cnt, float c, int wave,
                                        const float (&px)[kKlPerLane], const float (&py)[kKlPerLane],
                                        const float (&pz)[kKlPerLane], float (&S)[kKlPerLane],
                                        float (&V)[kKlPerLane][3], pcm_f4 *sTile) {
    for (int t0 = 0; t0 < cnt; t0 += kKlTile) {
        __syncthreads();  // the previous tile has been read
        const int cntT = min(kKlTile, cnt - t0);
        for (int p = threadIdx.x; p < cntT; p += kKlThreads) {  // a full tile is two points a thread
            pcm_f4 v;
            v.x = Q[pcm_at(L, t0 + p, 0)];
            v.y = Q[pcm_at(L, t0 + p, 1)];
            v.z = Q[pcm_at(L, t0 + p, 2)];
            v.w = 0.f;
            sTile[p] = v;
        }
        __syncthreads();
        const int end = min(cntT, (wave + 1) * kKlShare);
#pragma unroll 4
        for (int q = wave * kKlShare; q < end; ++q) {
            const pcm_f4 v = sTile[q];
#pragma unroll
            for (int r = 0; r < kKlPerLane; ++r) {
                const float dx = px[r] - v.x, dy = py[r] - v.y, dz = pz[r] - v.z;
                float k, g;
                kl_pair<K>(pcm_sqd(dx, dy, dz), c, k, g);
                S[r] += k;
                if constexpr (GRAD) {
                    V[r][0] = __builtin_fmaf(g, dx, V[r][0]);
                    V[r][1] = __builtin_fmaf(g, dy, V[r][1]);
                    V[r][2] = __builtin_fmaf(g, dz, V[r][2]);
                }
            }
        }
    }
}

// Rows blk * kKlRows .. of the cloud `own` (no points; the other cloud `oth`, nt points): the scan, the
// waves' merge and the outputs.  rowsum: the own cloud's first row of the element's (S_own, S_other)
// pairs; G: the own cloud's gradient of this element (GRAD).
template <int K, bool GRAD>
__device__ __forceinline__ void kl_block(const float *__restrict__ own, PcmLay Lo, int no,
                                         const float *__restrict__ oth, PcmLay Lt, int nt, int blk, float c,
                                         float coef_own, float coef_oth, float *__restrict__ G,
                                         float2 *__restrict__ rowsum, pcm_f4 *sTile) {
    constexpr int NA = GRAD ? 8 : 2;  // accumulators per row: S own, S other, V own, V other
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    float px[kKlPerLane], py[kKlPerLane], pz[kKlPerLane];
#pragma unroll
    for (int r = 0; r < kKlPerLane; ++r) {
        const int i = blk * kKlRows + r * 64 + lane;
        const int at = i < no ? i : 0;  // a lane past the cloud scans point 0 and writes nothing
        px[r] = own[pcm_at(Lo, at, 0)];
        py[r] = own[pcm_at(Lo, at, 1)];
        pz[r] = own[pcm_at(Lo, at, 2)];
    }
    float S0[kKlPerLane] = {}, S1[kKlPerLane] = {};
    float V0[kKlPerLane][3] = {}, V1[kKlPerLane][3] = {};
    kl_scan<K, GRAD>(own, Lo, no, c, wave, px, py, pz, S0, V0, sTile);
    kl_scan<K, GRAD>(oth, Lt, nt, c, wave, px, py, pz, S1, V1, sTile);

    __syncthreads();  // the last tile has been read: its storage takes the sums of waves 1..
    float *sAcc = (float *)sTile;  // [wave - 1][accumulator][row of the workgroup]
#pragma unroll
    for (int r = 0; r < kKlPerLane; ++r) {
        float a[8] = {S0[r], S1[r], V0[r][0], V0[r][1], V0[r][2], V1[r][0], V1[r][1], V1[r][2]};
        if (wave > 0) {
#pragma unroll
            for (int k = 0; k < NA; ++k) sAcc[((wave - 1) * NA + k) * kKlRows + r * 64 + lane] = a[k];
        }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int r = 0; r < kKlPerLane; ++r) {
        float a[8] = {S0[r], S1[r], V0[r][0], V0[r][1], V0[r][2], V1[r][0], V1[r][1], V1[r][2]};
#pragma unroll
        for (int w = 0; w < kKlWaves - 1; ++w) {  // (((s0 + s1) + s2) + ..) + s7
#pragma unroll
            for (int k = 0; k < NA; ++k) a[k] += sAcc[(w * NA + k) * kKlRows + r * 64 + lane];
        }
        const int i = blk * kKlRows + r * 64 + lane;
        if (i < no) {
            rowsum[i] = float2{a[0], a[1]};
            if constexpr (GRAD) {
                G[pcm_at(Lo, i, 0)] = __builtin_fmaf(coef_own, a[2], coef_oth * a[5]);
                G[pcm_at(Lo, i, 1)] = __builtin_fmaf(coef_own, a[3], coef_oth * a[6]);
                G[pcm_at(Lo, i, 2)] = __builtin_fmaf(coef_own, a[4], coef_oth * a[7]);
            }
        }
    }
}

struct KlCoefs {
    float c;                 // the exponent's scale
    float own1, oth1;        // fl(C a a), fl(-C a b): cloud 1's gradient from its V sums
    float own2, oth2;        // fl(C b b), fl(-C b a)
};

// element bid / (nblk1 + nblk2): its nblk1 row blocks of cloud 1, then the nblk2 of cloud 2
template <int K>
__global__ __launch_bounds__(kKlThreads) void kernel_loss_scan(const float *__restrict__ xyz1,
                                                               const float *__restrict__ xyz2, int n, int m,
                                                               int planes1, int planes2, int nblk1, int nblk2,
                                                               KlCoefs cf, float *__restrict__ gradxyz1,
                                                               float *__restrict__ gradxyz2,
                                                               float2 *__restrict__ rowsum) {
    __shared__ pcm_f4 sTile[kKlShared];
    int bi, blk;
    bool first;
    pcm_split_bm(pcm_xcd_remap(blockIdx.x, gridDim.x), nblk1, nblk2, bi, first, blk);
    const float *P1 = xyz1 + (size_t)bi * n * 3, *P2 = xyz2 + (size_t)bi * m * 3;
    const PcmLay L1 = pcm_lay(planes1, n), L2 = pcm_lay(planes2, m);
    float2 *R = rowsum + (size_t)bi * ((size_t)n + m);
    if (first) {
        float *G = gradxyz1 ? gradxyz1 + (size_t)bi * n * 3 : nullptr;
        if (G) kl_block<K, true>(P1, L1, n, P2, L2, m, blk, cf.c, cf.own1, cf.oth1, G, R, sTile);
        else kl_block<K, false>(P1, L1, n, P2, L2, m, blk, cf.c, cf.own1, cf.oth1, G, R, sTile);
    } else {
        float *G = gradxyz2 ? gradxyz2 + (size_t)bi * m * 3 : nullptr;
        if (G) kl_block<K, true>(P2, L2, m, P1, L1, n, blk, cf.c, cf.own2, cf.oth2, G, R + n, sTile);
        else kl_block<K, false>(P2, L2, m, P1, L1, n, blk, cf.c, cf.own2, cf.oth2, G, R + n, sTile);
    }
}

// loss_out[blockIdx.x] from the element's rows, in double: thread t adds rows t, t + 256, .. ascending,
// every wave its 64 threads by the six DPP steps, thread 0 the four waves' sums ascending
__global__ __launch_bounds__(kKlFinishThreads) void kernel_loss_finish(const float2 *__restrict__ rowsum, int n,
                                                                       int m, float *__restrict__ loss_out) {
    __shared__ double sWave[kKlFinishThreads / 64];
    const int rows = n + m;
    const float2 *R = rowsum + (size_t)blockIdx.x * rows;
    const double a = 1.0 / (double)n, b = 1.0 / (double)m;
    double acc = 0.0;
    for (int r = threadIdx.x; r < rows; r += kKlFinishThreads) {
        const float2 s = R[r];
        const double w = r < n ? a : b, wo = r < n ? b : a;
        acc += 0.5 * w * (w * (double)s.x - wo * (double)s.y);
    }
    const double wsum = pcm_wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) sWave[threadIdx.x >> 6] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < kKlFinishThreads / 64; ++w) total += sWave[w];
        loss_out[blockIdx.x] = (float)total;
    }
}

inline int kl_blocks(int n) { return (n + kKlRows - 1) / kKlRows; }

template <int K>
void kl_launch(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2, KlCoefs cf,
               float *gradxyz1, float *gradxyz2, float2 *rowsum, hipStream_t stream) {
    const int nblk1 = kl_blocks(n), nblk2 = kl_blocks(m);
    hipLaunchKernelGGL(kernel_loss_scan<K>, dim3((unsigned)(b * (nblk1 + nblk2))), dim3(kKlThreads), 0, stream, xyz1,
                       xyz2, n, m, layout1, layout2, nblk1, nblk2, cf, gradxyz1, gradxyz2, rowsum);
}

}  // namespace

extern "C" size_t pcm_kernel_loss_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return (size_t)b * ((size_t)n + (size_t)m) * sizeof(float2);
}

extern "C" int pcm_kernel_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                               int kernel, float blur, float *loss_out, float *gradxyz1, float *gradxyz2,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (b < 0 || n < 0 || m < 0) return PCM_ERR_INVALID_ARG;
    if ((layout1 != 0 && layout1 != 1) || (layout2 != 0 && layout2 != 1)) return PCM_ERR_INVALID_ARG;
    if (kernel < PCM_KERNEL_GAUSSIAN || kernel > PCM_KERNEL_ENERGY) return PCM_ERR_INVALID_ARG;
    if (!__builtin_isfinite(blur) || !(blur > 0.f)) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0 || m == 0 || !xyz1 || !xyz2 || !loss_out) return PCM_ERR_INVALID_ARG;
    if (n > kKlMaxN || m > kKlMaxN) return PCM_ERR_UNSUPPORTED;
    if ((long long)b * (kl_blocks(n) + kl_blocks(m)) > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;  // the grid
    if (!workspace || workspace_bytes < pcm_kernel_loss_workspace_bytes(b, n, m)) return PCM_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return PCM_ERR_INVALID_ARG;

    const double sigma = (double)blur, a = 1.0 / (double)n, bw = 1.0 / (double)m;
    const double log2e = 1.4426950408889634;
    double C;  // the kernel derivative's factor beside g (p - q)
    KlCoefs cf;
    if (kernel == PCM_KERNEL_GAUSSIAN) {
        cf.c = (float)(-log2e / (2.0 * sigma * sigma));
        C = -1.0 / (sigma * sigma);
    } else if (kernel == PCM_KERNEL_LAPLACIAN) {
        cf.c = (float)(-log2e / sigma);
        C = -1.0 / sigma;
    } else {
        cf.c = 0.f;
        C = -1.0;
    }
    cf.own1 = (float)(C * a * a);
    cf.oth1 = (float)(-C * a * bw);
    cf.own2 = (float)(C * bw * bw);
    cf.oth2 = (float)(-C * bw * a);

    float2 *rowsum = (float2 *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (kernel == PCM_KERNEL_GAUSSIAN)
        kl_launch<PCM_KERNEL_GAUSSIAN>(xyz1, xyz2, b, n, m, layout1, layout2, cf, gradxyz1, gradxyz2, rowsum, st);
    else if (kernel == PCM_KERNEL_LAPLACIAN)
        kl_launch<PCM_KERNEL_LAPLACIAN>(xyz1, xyz2, b, n, m, layout1, layout2, cf, gradxyz1, gradxyz2, rowsum, st);
    else
        kl_launch<PCM_KERNEL_ENERGY>(xyz1, xyz2, b, n, m, layout1, layout2, cf, gradxyz1, gradxyz2, rowsum, st);
    hipLaunchKernelGGL(kernel_loss_finish, dim3((unsigned)b), dim3(kKlFinishThreads), 0, st,
                       (const float2 *)rowsum, n, m, loss_out);
    return pcm_launch_status();
}
