// sampling.hip -- farthest point sampling for MI355X (gfx950, CDNA4): the whole
// chain of npoint dependent argmax reductions of one cloud in ONE launch.
//
// Replaces farthest_point_sample + index_points of the reference's
// utils/utils.py:316-360 as utils/datasets_sample_pcl.py:87-94 calls them for
// the 128- and 256-point ground truth: npoint iterations of 21 small device
// kernels each (torch.profiler's count), with a boolean-mask assignment that synchronises with the
// host every iteration.  DESIGN.md section 3.13 has the rationale and the numbers.
//
// One workgroup of T threads owns one cloud.  Lane t keeps points t, t + T, ..
// (P of them, P = the power of two >= ceil(n / T)) and their running minima in
// registers for the whole call; nothing of the state ever leaves them.  One
// iteration is a serial chain:
//   1. the current centroid's coordinates, fetched by index as a broadcast
//      read: from an LDS copy of the cloud (x[], y[], z[] planes) when the
//      instance's capacity T * P is at most kFpsLdsPoints, else a same-address
//      global read (the copy of 16384 points would need 192 KiB);
//   2. the update of the lane's P running minima (pcm_sqd, strict '<') and the
//      lane's best (value, index), lowest index on ties;
//   3. the wave's (max value, lowest index attaining it) by DPP: six steps for
//      the maximum, six for the lowest index among the lanes that hold it;
//   4. T > 64 only: lane 0 of each wave stores the wave's pair to its LDS slot,
//      ONE barrier, and every wave folds the slots (one read per lane, two or
//      four DPP steps a pass).  The slot arrays alternate by the iteration's parity --
//      the rule pcm_wg_or documents -- so a fast wave's next store never races a
//      slow wave's read.  T = 64 is one wave: no slots, no barrier.
// Lanes past a ragged n carry the value -1 (below every running minimum, which
// is >= 0 and never NaN) and their own index k >= n (loses every tie), so every
// reduction's result is a real point whatever bits the cloud holds.  No
// waiting between workgroups, no scratch, nothing but plain stores.
#include "pcm_common.h"
#include "pcm_internal.h"

namespace {

constexpr int kFpsMaxN = PCM_FPS_MAX_POINTS;
constexpr int kFpsLdsPoints = 8192;   // largest instance capacity whose copy (96 KiB) lives in LDS
constexpr float kFpsFar = 1e10f;      // utils/utils.py:346
constexpr float kFpsPad = -1.f;

typedef int fps_i2 __attribute__((ext_vector_type(2)));

// the steps of PCM_DPP_WAVE_STEPS that stay inside a row of 16 lanes: the
// result over lanes 0-3 in lane 3, over lanes 0-15 in lane 15
#define FPS_DPP_ROW4_STEPS(OP)                                                   \
    "s_nop 1\n\t" OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"      \
    "s_nop 1\n\t" OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf"
#define FPS_DPP_ROW16_STEPS(OP)                                                  \
    FPS_DPP_ROW4_STEPS(OP) "\n\t"                                                \
    "s_nop 1\n\t" OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"      \
    "s_nop 1\n\t" OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf"

// The wave's (max value, lowest index attaining it), returned wave-uniform:
// two passes of six one-instruction DPP steps (the helpers of pcm_common.h) --
// the maximum of the values, which are never NaN, then the minimum of the
// indices of the lanes that hold it.  A step on the (value, index) pair in the
// manner of pcm_wave_lexmin is two moves, three compares and two selects, all
// on the iteration's critical path: 605 against 400 ns per iteration at
// n = 1024.  `v == m` needs the maximum to be one lane's
// value bit for bit: the kernels run with float32 denormals preserved
// (.amdhsa_float_denorm_mode_32 3, hipcc's default for gfx950), so v_max_f32
// returns an input unchanged; values are never NaN.
__device__ __forceinline__ void fps_wave_lexmax(float &v, int &k) {
    const float m = pcm_wave_max_f32(v);
    int c = v == m ? k : 0x7fffffff;
    asm volatile(PCM_DPP_WAVE_STEPS("v_min_i32_dpp") : "+v"(c));
    k = __builtin_amdgcn_readlane(c, 63);
    v = m;
}

// the same over lanes 0 .. W - 1 of a wave's first row (W = 4 or 16 slots)
template <int W>
__device__ __forceinline__ void fps_row_lexmax(float &v, int &k) {
    static_assert(W == 4 || W == 16, "slots of a 256- or 1024-thread workgroup");
    float m = v;
    if constexpr (W == 16) asm volatile(FPS_DPP_ROW16_STEPS("v_max_f32_dpp") : "+v"(m));
    else asm volatile(FPS_DPP_ROW4_STEPS("v_max_f32_dpp") : "+v"(m));
    m = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), W - 1));
    int c = v == m ? k : 0x7fffffff;
    if constexpr (W == 16) asm volatile(FPS_DPP_ROW16_STEPS("v_min_i32_dpp") : "+v"(c));
    else asm volatile(FPS_DPP_ROW4_STEPS("v_min_i32_dpp") : "+v"(c));
    k = __builtin_amdgcn_readlane(c, W - 1);
    v = m;
}

// T threads, P points per lane: clouds of n <= T * P points, one per workgroup
template <int T, int P>
__global__ __launch_bounds__(T) void fps_kernel(const float *__restrict__ xyz, int n, int planes, int npoint,
                                                int start, long long *__restrict__ idx_out,
                                                float *__restrict__ sampled_out) {
    constexpr int kCap = T * P;
    constexpr bool kLds = kCap <= kFpsLdsPoints;
    constexpr int kW = T / 64;
    __shared__ float sP[kLds ? 3 * kCap : 1];   // x[kCap], y[kCap], z[kCap]
    __shared__ fps_i2 sSlot[2][kW];              // [parity][wave]: (value bits, index)

    const int tid = threadIdx.x;
    const PcmLay L = pcm_lay(planes, n);
    const float *Pc = xyz + (size_t)blockIdx.x * n * 3;
    long long *io = idx_out + (size_t)blockIdx.x * npoint;
    float *so = sampled_out ? sampled_out + (size_t)blockIdx.x * npoint * 3 : nullptr;

    float px[P], py[P], pz[P], run[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = j * T + tid;
        const bool real = k < n;
        px[j] = real ? Pc[pcm_at(L, k, 0)] : 0.f;
        py[j] = real ? Pc[pcm_at(L, k, 1)] : 0.f;
        pz[j] = real ? Pc[pcm_at(L, k, 2)] : 0.f;
        run[j] = real ? kFpsFar : kFpsPad;
        if constexpr (kLds) {
            sP[k] = px[j];
            sP[kCap + k] = py[j];
            sP[2 * kCap + k] = pz[j];
        }
    }
    if constexpr (kLds) {
        if constexpr (kW > 1) __syncthreads();
        else __builtin_amdgcn_wave_barrier();  // one wave: its LDS operations complete in order
    }

    int far = start;
    for (int i = 0; i < npoint; ++i) {
        float cx, cy, cz;
        if constexpr (kLds) {
            cx = sP[far];
            cy = sP[kCap + far];
            cz = sP[2 * kCap + far];
        } else {
            cx = Pc[pcm_at(L, far, 0)];
            cy = Pc[pcm_at(L, far, 1)];
            cz = Pc[pcm_at(L, far, 2)];
        }
        if (tid == 0) {
            io[i] = far;
            if (so) {
                so[3 * (size_t)i + 0] = cx;
                so[3 * (size_t)i + 1] = cy;
                so[3 * (size_t)i + 2] = cz;
            }
        }
        // a NaN distance fails '<' and changes nothing; a padding slot stays -1 (d >= 0 or NaN)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const float d = pcm_sqd(px[j] - cx, py[j] - cy, pz[j] - cz);
            run[j] = d < run[j] ? d : run[j];
        }
        // the lane's best, seeded with its first slot; strict '>' keeps the lowest index
        float bv = run[0];
        int bk = tid;
#pragma unroll
        for (int j = 1; j < P; ++j) {
            const bool take = run[j] > bv;
            bv = take ? run[j] : bv;
            bk = take ? j * T + tid : bk;
        }
        fps_wave_lexmax(bv, bk);
        if constexpr (kW > 1) {
            fps_i2 *slot = sSlot[i & 1];
            if ((tid & 63) == 0) slot[tid >> 6] = fps_i2{__float_as_int(bv), bk};
            __syncthreads();
            const fps_i2 s = slot[tid & (kW - 1)];
            bv = __int_as_float(s.x);
            bk = s.y;
            fps_row_lexmax<kW>(bv, bk);
        }
        // in range by the argument above; the clamp keeps the next read inside the cloud regardless
        far = min(bk, n - 1);
    }
}

typedef void (*fps_kernel_t)(const float *, int, int, int, int, long long *, float *);

// the instance of T threads for n points: the smallest P (a power of two) with T * P >= n
template <int T>
fps_kernel_t fps_instance(int n) {
    const int need = (n + T - 1) / T;
    if (need <= 1) return fps_kernel<T, 1>;
    if (need <= 2) return fps_kernel<T, 2>;
    if (need <= 4) return fps_kernel<T, 4>;
    if (need <= 8) return fps_kernel<T, 8>;
    if (need <= 16) return fps_kernel<T, 16>;
    if constexpr (T < 1024) {  // 1024 threads are four waves per SIMD: 128 registers a lane
        if (need <= 32) return fps_kernel<T, 32>;
        if (need <= 64) return fps_kernel<T, 64>;
    }
    return nullptr;
}

// Workgroup size by cloud size, from tools/bench_fps.py --sweep on one MI355X
// (profiles/fps/bench_fps_sweep_run1.txt), ns per iteration at
// 64 / 256 / 1024 threads: n = 512: 334 / 344 / 453 -- one wave pays for
// having no barrier up to eight points a lane; n = 1024: 516 / 400 / 455 and
// n = 2048: 880 / 491 / 520; n = 4096: 2013 / 675 / 649 and n = 16384:
// - / 2225 / 1449.
inline int fps_default_threads(int n) {
    if (n <= 512) return 64;
    if (n <= 2048) return 256;
    return 1024;
}

int fps_check(const float *xyz, int b, int n, int layout, int npoint, int start, const int64_t *idx_out) {
    if (b < 0 || n < 0 || npoint < 0) return PCM_ERR_INVALID_ARG;
    if (layout != 0 && layout != 1) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0 || npoint == 0) return PCM_ERR_INVALID_ARG;
    if (start < 0 || start >= n) return PCM_ERR_INVALID_ARG;
    if (!xyz || !idx_out) return PCM_ERR_INVALID_ARG;
    if (n > kFpsMaxN) return PCM_ERR_UNSUPPORTED;
    return 1;  // a launch is due
}

int fps_launch(int threads, const float *xyz, int b, int n, int layout, int npoint, int start, int64_t *idx_out,
               float *sampled_out, void *stream) {
    const int st = fps_check(xyz, b, n, layout, npoint, start, idx_out);
    if (st <= 0) return st;
    fps_kernel_t kern = nullptr;
    if (threads == 64) kern = fps_instance<64>(n);
    else if (threads == 256) kern = fps_instance<256>(n);
    else if (threads == 1024) kern = fps_instance<1024>(n);
    else return PCM_ERR_INVALID_ARG;
    if (!kern) return PCM_ERR_UNSUPPORTED;  // a forced size too small for the cloud
    hipLaunchKernelGGL(kern, dim3((unsigned)b), dim3((unsigned)threads), 0, (hipStream_t)stream, xyz, n, layout,
                       npoint, start, (long long *)idx_out, sampled_out);
    return pcm_launch_status();
}

}  // namespace

extern "C" int pcm_fps(const float *xyz, int b, int n, int layout, int npoint, int start, int64_t *idx_out,
                       float *sampled_out, void *stream) {
    return fps_launch(fps_default_threads(n < 1 ? 1 : n), xyz, b, n, layout, npoint, start, idx_out, sampled_out,
                      stream);
}

extern "C" int pcm_tune_fps(int threads, const float *xyz, int b, int n, int layout, int npoint, int start,
                            int64_t *idx_out, float *sampled_out, void *stream) {
    return fps_launch(threads, xyz, b, n, layout, npoint, start, idx_out, sampled_out, stream);
}

extern "C" int pcm_tune_fps_default_threads(int n) {
    return fps_default_threads(n);
}
