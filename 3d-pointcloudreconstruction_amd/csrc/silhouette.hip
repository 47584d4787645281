// silhouette.hip -- projection loss for MI355X (gfx950, CDNA4): the Gaussian-
// splatted silhouette of a point cloud, its backward, and the 'bce_prob'
// projection loss with its gradient.
//
// Replaces, for finetune.py:154-162, cont_proj of the reference's
// utils/projection.py:4-67 (a B x N x H x W x 2 float32 difference tensor, its
// exponential, a B x N x H x W product and a sum over N -- on the CPU,
// utils/utils.py:232) and the 'bce_prob' branch of loss/proj_loss.py:17-19 with
// the mean of :43.  DESIGN.md section 3.12 has the rationale and the numbers.
//
// The splat is separable: S[b,h,w] = sum_n ex[n,h] ey[n,w] with
// ex[n,h] = exp(-(gx_n - h)^2 / (2 sigma^2)), so a point costs grid_h + grid_w
// exponentials and the rest is a rank-N outer-product accumulation.
//
// Forward kernel: a workgroup of kSilW waves owns one 32 x 32 tile of one
// cloud's grid.  The points go through LDS in chunks of kSilChunk: every
// thread forms four of the chunk's factors at a time (one v_exp_f32 each) and
// stores them as one 16-byte word, consecutive lanes to consecutive words;
// then wave w accumulates points [16 w, 16 w + 16) of the chunk, each lane into
// a 4 x 4 register tile of cells from two 16-byte LDS reads per point (eight
// packed FMAs).  The waves' partial tiles are added through LDS in ascending
// wave order.  The order of a cell's sum depends on n alone -- not on the
// tile, the batch size or the cloud's place in the batch.
//
// Backward kernel: a workgroup owns kSilBwdT / SL points of one cloud, SL =
// the grid's columns in slices of eight.  Thread (slice, point) keeps its
// point's eight ey / d ey factors in registers and walks the rows of G, staged
// through LDS in bands of 32 rows together with the band's ex / d ex factors
// of every point; the slices' partial sums are added through LDS in ascending
// slice order.  Nothing of size N x H x W exists anywhere.
//
// Projection loss: one thread per eight strided elements, DPP wave sum, the
// waves in order, one partial per workgroup; a second one-workgroup launch
// adds the partials (a single workgroup writes the loss itself).  The kernel
// boundary is the hand-off: no tickets, no polling, no atomics.
#include "pcm_common.h"
#include "chamfer_loss.h"

using pcm_loss::wave_sum;

namespace {

constexpr int kSilMaxGrid = PCM_SILHOUETTE_MAX_GRID;  // rows or columns of the silhouette
constexpr int kSilW = 8;                              // waves per forward workgroup
constexpr int kSilT = 64 * kSilW;
constexpr int kSilTile = 32;                          // cells per tile side
constexpr int kSilPPW = 16;                           // points per wave per chunk
constexpr int kSilBatch = 8;                          // points whose LDS operands are in flight together
constexpr int kSilChunk = kSilW * kSilPPW;            // points per LDS chunk
constexpr int kSilRow = 2 * kSilTile;                 // floats per staged point: ex[32], ey[32]
constexpr int kSilFill = kSilChunk * kSilRow / 4 / kSilT;  // 16-byte words per thread per chunk
static_assert(kSilChunk * kSilRow / 4 % kSilT == 0, "whole words per thread");
static_assert(kSilW * kSilTile * kSilTile <= kSilChunk * kSilRow, "the partial tiles reuse the staging buffer");

// exp(-(d*d) / (2 sigma^2)) as one hardware exponential: c = -log2(e) / (2 sigma^2).
// NaN stays NaN; d = +-inf gives exp2(-inf) = 0.
__device__ __forceinline__ float sil_factor(float d, float c) {
    return __builtin_amdgcn_exp2f((d * d) * c);
}

// pinned coordinate map of projection.py:20-21
__device__ __forceinline__ float sil_coord(float p, int grid) {
    return ((p + 1.f) * (float)grid) / 2.f;
}

__global__ __launch_bounds__(kSilT) void silhouette_fwd_kernel(const float *__restrict__ xyz, int n, int planes,
                                                               int grid_h, int grid_w, int tiles_h, int tiles_w,
                                                               float c, float *__restrict__ sil) {
    __shared__ __attribute__((aligned(16))) float sE[kSilChunk * kSilRow];  // 32 KiB

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int per = tiles_h * tiles_w;
    const int cloud = (int)blockIdx.x / per;
    const int tile = (int)blockIdx.x - cloud * per;
    const int h0 = (tile / tiles_w) * kSilTile;
    const int w0 = (tile % tiles_w) * kSilTile;
    const PcmLay L = pcm_lay(planes, n);
    const float *P = xyz + (size_t)cloud * n * 3;

    // staging role: word f4 (of 16) of the rows of points pl + 32 r; words 0-7
    // are ex (first coordinate, rows h0 + 4 f4 ..), words 8-15 ey
    const int f4 = tid & 15;
    const int pl = tid >> 4;
    const int comp = f4 >> 3;
    const int cell0 = (comp ? w0 : h0) + (f4 & 7) * 4;
    const int gdim = comp ? grid_w : grid_h;

    // accumulating role: cells (h0 + 4 ty + r, w0 + 4 tx + q)
    const int ty = lane >> 3, tx = lane & 7;
    pcm_f2 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r][0] = acc[r][1] = pcm_f2{0.f, 0.f};

    float cur[kSilFill], nxt[kSilFill];
#pragma unroll
    for (int r = 0; r < kSilFill; ++r) {
        const int p = pl + 32 * r;
        cur[r] = p < n ? P[pcm_at(L, p, comp)] : 0.f;
    }
    for (int base = 0; base < n; base += kSilChunk) {
        // the next chunk's coordinates travel while this one is consumed
#pragma unroll
        for (int r = 0; r < kSilFill; ++r) {
            const int p = base + kSilChunk + pl + 32 * r;
            nxt[r] = p < n ? P[pcm_at(L, p, comp)] : 0.f;
        }
        if (base > 0) __syncthreads();  // previous chunk fully consumed
#pragma unroll
        for (int r = 0; r < kSilFill; ++r) {
            const int p = base + pl + 32 * r;
            pcm_f4 v = pcm_f4{0.f, 0.f, 0.f, 0.f};  // a point past n adds 0 * 0
            if (p < n) {
                const float g = sil_coord(cur[r], gdim);
                v.x = sil_factor(g - (float)(cell0 + 0), c);
                v.y = sil_factor(g - (float)(cell0 + 1), c);
                v.z = sil_factor(g - (float)(cell0 + 2), c);
                v.w = sil_factor(g - (float)(cell0 + 3), c);
            }
            *reinterpret_cast<pcm_f4 *>(&sE[(pl + 32 * r) * kSilRow + f4 * 4]) = v;
        }
        __syncthreads();
        const float *row = &sE[wave * kSilPPW * kSilRow];
        // eight points' operands are requested before the first is used: one LDS
        // latency per eight points, not one per point (the order of the sum is j's)
#pragma unroll
        for (int j0 = 0; j0 < kSilPPW; j0 += kSilBatch) {
            pcm_f4 a[kSilBatch], e[kSilBatch];
#pragma unroll
            for (int j = 0; j < kSilBatch; ++j) {
                a[j] = *reinterpret_cast<const pcm_f4 *>(row + (j0 + j) * kSilRow + 4 * ty);
                e[j] = *reinterpret_cast<const pcm_f4 *>(row + (j0 + j) * kSilRow + kSilTile + 4 * tx);
            }
#pragma unroll
            for (int j = 0; j < kSilBatch; ++j) {
                const float ar[4] = {a[j].x, a[j].y, a[j].z, a[j].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const pcm_f2 s = pcm_f2{ar[r], ar[r]};
                    acc[r][0] = __builtin_elementwise_fma(s, e[j].xy, acc[r][0]);
                    acc[r][1] = __builtin_elementwise_fma(s, e[j].zw, acc[r][1]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kSilFill; ++r) cur[r] = nxt[r];
    }

    // ---- the waves' partial tiles, added in ascending wave order
    __syncthreads();
    float *part = sE;  // [kSilW][32 * 32]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pcm_f4 v;
        v.xy = acc[r][0];
        v.zw = acc[r][1];
        *reinterpret_cast<pcm_f4 *>(&part[wave * kSilTile * kSilTile + (4 * ty + r) * kSilTile + 4 * tx]) = v;
    }
    __syncthreads();
    float *out = sil + (size_t)cloud * grid_h * grid_w;
#pragma unroll
    for (int i = 0; i < kSilTile * kSilTile / kSilT; ++i) {
        const int cell = tid + i * kSilT;
        float s = part[cell];
#pragma unroll
        for (int w = 1; w < kSilW; ++w) s += part[w * kSilTile * kSilTile + cell];
        const int h = h0 + cell / kSilTile, wc = w0 + cell % kSilTile;
        if (h < grid_h && wc < grid_w) out[(size_t)h * grid_w + wc] = s;
    }
}

constexpr int kSilBwdT = 256;      // most threads of a backward workgroup
constexpr int kSilBwdMaxP = 64;    // most points of a backward workgroup
constexpr int kSilBand = 32;       // rows of G staged at a time
constexpr int kSilSlice = 8;       // columns per thread
constexpr int kSilBwdBatch = 8;    // rows whose LDS operands are in flight together

// slices per point for grid_w columns: 1, 2, 4, 8 or 16 (eight columns each)
inline int sil_bwd_slices(int grid_w) {
    int sl = 1;
    while (sl * kSilSlice < grid_w) sl *= 2;
    return sl;
}
inline int sil_bwd_points(int sl) {
    const int p = kSilBwdT / sl;
    return p < kSilBwdMaxP ? p : kSilBwdMaxP;
}

// P points x SL slices threads (tid = slice * P + point), both powers of two
__global__ __launch_bounds__(kSilBwdT) void silhouette_bwd_kernel(const float *__restrict__ xyz, int n, int planes,
                                                                 int grid_h, int grid_w, int P, int SL, int nblk,
                                                                 float c, float inv_sigma_sq,
                                                                 const float *__restrict__ grad_sil,
                                                                 float *__restrict__ gradxyz) {
    __shared__ __attribute__((aligned(16))) float sG[kSilBand * kSilMaxGrid];  // 16 KiB: [32][SL * 8]
    __shared__ float sEx[kSilBand * kSilBwdMaxP];                              // 8 KiB: [32][P]
    __shared__ float sDex[kSilBand * kSilBwdMaxP];                             // 8 KiB
    __shared__ float sPart[2][kSilBwdT];                                       // [x | y][slice * P + point]

    const int tid = threadIdx.x;
    const int nthreads = P * SL;
    const int pt = tid & (P - 1);
    const int slice = tid / P;
    const int cloud = (int)blockIdx.x / nblk;
    const int blk = (int)blockIdx.x - cloud * nblk;
    const int p = blk * P + pt;
    const bool valid = p < n;
    const PcmLay L = pcm_lay(planes, n);
    const float *Pc = xyz + (size_t)cloud * n * 3;
    const float *G = grad_sil + (size_t)cloud * grid_h * grid_w;
    const int WP = SL * kSilSlice;  // padded row of the staged band

    float gx = 0.f, gy = 0.f;
    if (valid) {
        gx = sil_coord(Pc[pcm_at(L, p, 0)], grid_h);
        gy = sil_coord(Pc[pcm_at(L, p, 1)], grid_w);
    }
    // this thread's eight columns: ey and d ey / d gy
    pcm_f2 ey[kSilSlice / 2], dey[kSilSlice / 2];
#pragma unroll
    for (int k = 0; k < kSilSlice; k += 2) {
        const float d0 = gy - (float)(slice * kSilSlice + k), d1 = gy - (float)(slice * kSilSlice + k + 1);
        const float e0 = sil_factor(d0, c), e1 = sil_factor(d1, c);
        ey[k / 2] = pcm_f2{e0, e1};
        dey[k / 2] = pcm_f2{(-d0 * inv_sigma_sq) * e0, (-d1 * inv_sigma_sq) * e1};
    }

    float ax = 0.f, ay = 0.f;
    for (int hb = 0; hb < grid_h; hb += kSilBand) {
        if (hb > 0) __syncthreads();  // previous band fully consumed
        // the band of G, zero beyond the grid's rows and columns
        for (int i = tid; i < kSilBand * WP; i += nthreads) {
            const int r = i / WP, col = i - r * WP;
            const int h = hb + r;
            sG[i] = (h < grid_h && col < grid_w) ? G[(size_t)h * grid_w + col] : 0.f;
        }
        // the band's ex and d ex / d gx of this thread's point, rows slice, slice + SL, ..
        for (int r = slice; r < kSilBand; r += SL) {
            const float d = gx - (float)(hb + r);
            const float e = sil_factor(d, c);
            sEx[r * P + pt] = e;
            sDex[r * P + pt] = (-d * inv_sigma_sq) * e;
        }
        __syncthreads();
        const float *g = &sG[slice * kSilSlice];
        // kSilBwdBatch rows' operands are requested before the first is used
        // (one LDS latency per batch); the sums run over r in ascending order
#pragma unroll 1
        for (int r0 = 0; r0 < kSilBand; r0 += kSilBwdBatch) {
            pcm_f4 g0[kSilBwdBatch], g1[kSilBwdBatch];
            float te[kSilBwdBatch], td[kSilBwdBatch];
#pragma unroll
            for (int k = 0; k < kSilBwdBatch; ++k) {
                g0[k] = *reinterpret_cast<const pcm_f4 *>(g + (r0 + k) * WP);
                g1[k] = *reinterpret_cast<const pcm_f4 *>(g + (r0 + k) * WP + 4);
                te[k] = sEx[(r0 + k) * P + pt];
                td[k] = sDex[(r0 + k) * P + pt];
            }
#pragma unroll
            for (int k = 0; k < kSilBwdBatch; ++k) {
                pcm_f2 u = g0[k].xy * ey[0];
                pcm_f2 v = g0[k].xy * dey[0];
                u = __builtin_elementwise_fma(g0[k].zw, ey[1], u);
                v = __builtin_elementwise_fma(g0[k].zw, dey[1], v);
                u = __builtin_elementwise_fma(g1[k].xy, ey[2], u);
                v = __builtin_elementwise_fma(g1[k].xy, dey[2], v);
                u = __builtin_elementwise_fma(g1[k].zw, ey[3], u);
                v = __builtin_elementwise_fma(g1[k].zw, dey[3], v);
                ax = __builtin_fmaf(td[k], u.x + u.y, ax);
                ay = __builtin_fmaf(te[k], v.x + v.y, ay);
            }
        }
    }

    // ---- the slices' partial sums, added in ascending slice order
    sPart[0][tid] = ax;
    sPart[1][tid] = ay;
    __syncthreads();
    if (slice == 0 && valid) {
        float sx = sPart[0][pt], sy = sPart[1][pt];
        for (int s = 1; s < SL; ++s) {
            sx += sPart[0][s * P + pt];
            sy += sPart[1][s * P + pt];
        }
        float *o = gradxyz + (size_t)cloud * n * 3;
        o[pcm_at(L, p, 0)] = ((float)grid_h / 2.f) * sx;
        o[pcm_at(L, p, 1)] = ((float)grid_w / 2.f) * sy;
        o[pcm_at(L, p, 2)] = 0.f;
    }
}

constexpr int kBceT = 256;                  // threads per workgroup
constexpr int kBcePer = 8;                  // elements per thread
constexpr int kBceBlock = kBceT * kBcePer;  // elements per workgroup

inline long long bce_blocks(long long count) { return (count + kBceBlock - 1) / kBceBlock; }

// the workgroup's sum: DPP wave sums, then the waves in ascending order (valid in thread 0)
__device__ __forceinline__ float bce_wg_sum(float v, float *sRed) {
    const float ws = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = ws;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kBceT / 64; ++w) s += sRed[w];
    }
    return s;
}

// workgroup k: elements [2048 k, 2048 k + 2048), thread t the elements t + 256 j
__global__ __launch_bounds__(kBceT) void proj_bce_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                         long long count, float w, float *__restrict__ grad_pred,
                                                         float *__restrict__ partials, float *__restrict__ loss_out) {
    __shared__ float sRed[kBceT / 64];
    const long long base = (long long)blockIdx.x * kBceBlock + threadIdx.x;
    float pv[kBcePer], gv[kBcePer];
#pragma unroll
    for (int j = 0; j < kBcePer; ++j) {
        const long long i = base + (long long)j * kBceT;
        pv[j] = i < count ? pred[i] : 0.f;
        gv[j] = i < count ? gt[i] : 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kBcePer; ++j) {
        const long long i = base + (long long)j * kBceT;
        if (i < count) {
            // proj_loss.py:17-19, in float32 and in this order
            const float a = pv[j] + 1e-8f;
            const float q = (1.f - pv[j]) - 1e-8f;
            const float cc = fabsf(q);
            const float term = ((-gv[j]) * logf(a)) * w - (1.f - gv[j]) * logf(cc);
            s += term;
            if (grad_pred) {
                // two quotients of opposite sign can cancel: formed in double, rounded once
                const double t = -((double)gv[j] * (double)w) / (double)a + (1.0 - (double)gv[j]) / (double)q;
                grad_pred[i] = (float)(t / (double)(float)count);
            }
        }
    }
    const float tot = bce_wg_sum(s, sRed);
    if (threadIdx.x == 0) {
        if (loss_out) loss_out[0] = tot / (float)count;  // a single workgroup: the loss itself
        else partials[blockIdx.x] = tot;
    }
}

// one workgroup: thread t adds partials t, t + 256, .. in order, then the workgroup's sum
__global__ __launch_bounds__(kBceT) void proj_bce_finalize_kernel(const float *__restrict__ partials, long long nblk,
                                                                  long long count, float *__restrict__ loss_out) {
    __shared__ float sRed[kBceT / 64];
    float s = 0.f;
    for (long long k = threadIdx.x; k < nblk; k += kBceT) s += partials[k];
    const float tot = bce_wg_sum(s, sRed);
    if (threadIdx.x == 0) loss_out[0] = tot / (float)count;
}

int sil_check(const float *xyz, int b, int n, int layout, int grid_h, int grid_w, float sigma_sq, const void *p1,
              const void *p2) {
    if (b < 0 || n < 0) return PCM_ERR_INVALID_ARG;
    if (layout != 0 && layout != 1) return PCM_ERR_INVALID_ARG;
    if (grid_h < 1 || grid_w < 1) return PCM_ERR_INVALID_ARG;
    if (!(sigma_sq > 0.f) || !__builtin_isfinite(sigma_sq)) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0) return PCM_ERR_INVALID_ARG;
    if (!xyz || !p1 || !p2) return PCM_ERR_INVALID_ARG;
    if (grid_h > kSilMaxGrid || grid_w > kSilMaxGrid) return PCM_ERR_UNSUPPORTED;
    return 1;  // a launch is due
}

// -log2(e) / (2 sigma^2): formed in double, rounded once
inline float sil_exp2_scale(float sigma_sq) { return (float)(-1.4426950408889634 / (2.0 * (double)sigma_sq)); }

}  // namespace

extern "C" int pcm_silhouette_forward(const float *xyz, int b, int n, int layout, int grid_h, int grid_w,
                                      float sigma_sq, float *sil, void *stream) {
    const int st = sil_check(xyz, b, n, layout, grid_h, grid_w, sigma_sq, sil, sil);
    if (st <= 0) return st;
    const int tiles_h = (grid_h + kSilTile - 1) / kSilTile, tiles_w = (grid_w + kSilTile - 1) / kSilTile;
    const long long blocks = (long long)b * tiles_h * tiles_w;
    if (blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(silhouette_fwd_kernel, dim3((unsigned)blocks), dim3(kSilT), 0, (hipStream_t)stream, xyz, n,
                       layout, grid_h, grid_w, tiles_h, tiles_w, sil_exp2_scale(sigma_sq), sil);
    return pcm_launch_status();
}

extern "C" int pcm_silhouette_backward(const float *xyz, int b, int n, int layout, int grid_h, int grid_w,
                                       float sigma_sq, const float *grad_sil, float *gradxyz, void *stream) {
    const int st = sil_check(xyz, b, n, layout, grid_h, grid_w, sigma_sq, grad_sil, gradxyz);
    if (st <= 0) return st;
    const int SL = sil_bwd_slices(grid_w), P = sil_bwd_points(SL);
    const int nblk = (n + P - 1) / P;
    const long long blocks = (long long)b * nblk;
    if (blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(silhouette_bwd_kernel, dim3((unsigned)blocks), dim3(P * SL), 0, (hipStream_t)stream, xyz, n,
                       layout, grid_h, grid_w, P, SL, nblk, sil_exp2_scale(sigma_sq), 1.f / sigma_sq, grad_sil,
                       gradxyz);
    return pcm_launch_status();
}

extern "C" size_t pcm_proj_bce_workspace_bytes(long long count) {
    if (count <= 0) return 0;
    const size_t bytes = (size_t)bce_blocks(count) * sizeof(float);
    return (bytes + 127) / 128 * 128;
}

extern "C" int pcm_proj_bce(const float *pred, const float *gt, long long count, float w, float *loss_out,
                            float *grad_pred, void *workspace, size_t workspace_bytes, void *stream) {
    if (count < 0) return PCM_ERR_INVALID_ARG;
    if (count == 0) return PCM_OK;
    if (!pred || !gt || !loss_out) return PCM_ERR_INVALID_ARG;
    const long long nblk = bce_blocks(count);
    if (nblk > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < pcm_proj_bce_workspace_bytes(count)) return PCM_ERR_WORKSPACE;
    float *partials = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(proj_bce_kernel, dim3((unsigned)nblk), dim3(kBceT), 0, st, pred, gt, count, w, grad_pred,
                       partials, nblk == 1 ? loss_out : (float *)nullptr);
    if (nblk > 1)
        hipLaunchKernelGGL(proj_bce_finalize_kernel, dim3(1), dim3(kBceT), 0, st, partials, nblk, count, loss_out);
    return pcm_launch_status();
}
