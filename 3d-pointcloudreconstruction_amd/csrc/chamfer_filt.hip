// chamfer_filt.hip -- Chamfer3D forward, filtered form, and the fused
// loss + gradient kernel (gfx950).
//
// Same results as NmDistanceKernel (metric/chamfer3D/chamfer3D.cu:12-134): per
// query the minimum of the pinned squared distance fma(dz,dz,fma(dy,dy,dx*dx))
// over the other cloud and the LOWEST index attaining it, bit-identical.  What
// changes is how the minimum is found:
//
//   1. Filter.  The workgroup stages the target cloud in LDS as
//      (u, w) = (-2 t', |t'|^2), t' = t - c (c = mean of the workgroup's
//      queries), and every lane evaluates a(q, t) = |t'|^2 - 2 q'.t' with
//      three packed FMAs per two candidates (v_pk_fma_f32) -- 1.5 VALU
//      instructions per pair plus the min fold, against 3 for the exact
//      difference form.  Per query it keeps the best chunk (C candidates) and
//      the best value of any OTHER chunk ("second"), one v_med3 per chunk.
//   2. Proof.  a + |q'|^2 differs from the exact fp32 distance by at most
//      E = 16 u (R + |q'|)^2 (u = 2^-24, R = max |t'| over the targets; the
//      bound sums the rounding of w and the three FMAs (6u), the centering
//      (2u) and the exact formula's own rounding (5u)).  If second - best > 2E,
//      every candidate outside the best chunk is provably farther than the
//      best chunk's minimum, so the exact answer (value and lowest index) lies
//      in that chunk.
//   3. Exact rescan of that chunk with the pinned formula on the original
//      coordinates (from LDS when the cloud is one tile); queries whose gap is
//      within 2E (near-ties, ~0.1 % of random queries) get a cooperative exact
//      scan of the whole cloud by the workgroup, several queries per pass.
//
// Non-finite coordinates divert the workgroup to the reference-exact 512-tile
// scan (NaN placement depends on the reference's tile boundaries).
//
// Fused loss + gradient (pcm_chamfer_loss_grad): the training step of
// loss/loss.py:31-37 and its backward (chamfer3D.cu:155-195) in ONE launch
// (default: the granule hand-off, kGran).  A workgroup owns 256 queries of one
// (batch element, direction).  It runs its forward share and publishes every
// argmin as an 8-byte {call tag, idx} granule (one sc1 store: the data is its
// own flag, MI355X_MICROARCH.md handoff-1to1) and its partial distance sum as
// a {tag, sum} granule.  It then computes the gradients of its OWN query
// range: it sweeps the granules it needs (its range's argmins and the other
// direction's), waiting -- bounded -- only on its own batch element's
// workgroups, buckets the sources by target in LDS and sums them in ascending
// source order, in the reference's kernel order (identical bits to
// pcm_chamfer_backward fed graddist = w).  The grid's last workgroup sweeps
// the partial granules and sums them in a fixed order (deterministic means).
// Granules of earlier calls carry older tags, so the workspace is never
// re-zeroed; a timed-out wait recomputes the missing argmins locally (time,
// never correctness).  Variants 11/12 (round 4; tested, not the default)
// read the gradient phase's clouds from the forward's own LDS (its resident
// target tile and its queries) instead of copying both clouds in; 12 also
// stages the target tile in parts so the scan starts before the prologue's
// loads have all landed.  tools/ab_chamfer.py, same box: 7 13.65-13.74 us,
// 11 13.62-13.77 us, 12 13.80-13.99 us (gpurun_out r04e).
#include <type_traits>

#include "pcm_common.h"
#include "pcm_internal.h"
#include "chamfer_loss.h"

namespace {
using namespace pcm_loss;

constexpr float kFiltU16 = 9.5367431640625e-07f;  // 16 u = 2^-20 (bound derivation above)

// Phase stamps for tools/stamp_filt.py (profiling build only: make stamps).
// Thread 0 of every workgroup records s_memrealtime (100 MHz) at 8 points.
#ifdef PCM_STAMPS
constexpr int kStampSlots = 1 << 16;
__device__ unsigned long long g_pcm_stamps[kStampSlots * 8];
#define PCM_STAMP(i)                                                                           \
    do {                                                                                       \
        if (threadIdx.x == 0 && blockIdx.x < kStampSlots)                                      \
            g_pcm_stamps[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime();            \
    } while (0)
// the fused kernel's own 8 stamps go to the table's upper half
#define PCM_STAMP2(i)                                                                          \
    do {                                                                                       \
        if (threadIdx.x == 0 && blockIdx.x < kStampSlots / 2)                                  \
            g_pcm_stamps[(kStampSlots / 2 + blockIdx.x) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define PCM_STAMP(i) \
    do {             \
    } while (0)
#define PCM_STAMP2(i) \
    do {              \
    } while (0)
#endif

// The workgroup's LDS arena: one static array per size, shared by every
// phase of a kernel that asks for the same size.
template <int kBytes, int kTag = 0>
__device__ __forceinline__ unsigned char *lds_arena() {
    __shared__ __attribute__((aligned(16))) unsigned char arena[kBytes];
    return arena;
}

// an LDS-DMA issued by filt_forward once its first target tile is staged:
// the copy lands while the scan runs (the scan makes no global loads)
struct PreDma {
    void *dst1;
    const void *src1;
    int bytes1;
    void *dst2;
    const void *src2;
    int bytes2;
};

// Arena bytes of the filtered forward: the scan tile (u, w), then -- after the
// scan, in the same bytes -- the raw target cloud (single-tile clouds) and the
// per-wave merge arrays.
template <int W, int QPT, int TILE>
struct FiltLds {
    static constexpr int kScan = 4 * TILE * 4;
    static constexpr int kTail = 4 * TILE * 4 + 3 * W * 64 * QPT * 4;
    static constexpr int kBytes = kScan > kTail ? kScan : kTail;
};

// Raw-tile slot of point p in the filtered forward's LDS copy of a resident
// target cloud: rotated by its chunk index inside the chunk, so the rescan's
// lanes -- one query each, random chunks -- spread over the 16 four-bank
// groups a ds_read_b128 lane group uses, not one.
template <int C>
__device__ __forceinline__ int filt_slot(int p) {
    static_assert((C & (C - 1)) == 0, "chunk is a power of two");
    return (p & ~(C - 1)) | ((p + (int)((unsigned)p / C)) & (C - 1));  // p >= 0
}

// forward outputs: plain stores, or write-through (sc1) when another
// workgroup of the same launch reads them (fused loss + gradient)
template <bool kSc1, typename Tv>
__device__ __forceinline__ void out_st(Tv *p, Tv v) {
    if constexpr (kSc1) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// Sum over the wave by DPP steps (pcm_common.h), returned wave-uniform.
__device__ __forceinline__ float wave_sum_dpp(float v) {
    asm volatile(PCM_DPP_WAVE_STEPS("v_add_f32_dpp") : "+v"(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_sum_dpp(int v) {
    asm volatile(PCM_DPP_WAVE_STEPS("v_add_u32_dpp") : "+v"(v));
    return __builtin_amdgcn_readlane(v, 63);
}

// One 4-candidate group against four queries (QPT = 4): the 24 packed FMAs
// of a(q, t) = fma(qx, ux, fma(qy, uy, fma(qz, uz, w))) for 8 independent
// (query, candidate pair) chains issued stage by stage, then the min folds.
// Left to itself hipcc interleaves only two chains in most groups and each
// FMA waits on its predecessor; the arithmetic here is the same, in the same
// order.
__device__ __forceinline__ void filt_group4(float (&mn)[4], const pcm_f2 (&px)[4], const pcm_f2 (&py)[4],
                                            const pcm_f2 (&pz)[4], pcm_f4 X4, pcm_f4 Y4, pcm_f4 Z4, pcm_f4 W4) {
    const pcm_f2 xa = X4.xy, xb = X4.zw, ya = Y4.xy, yb = Y4.zw, za = Z4.xy, zb = Z4.zw, wa = W4.xy, wb = W4.zw;
    pcm_f2 a0, a1, a2, a3, b0, b1, b2, b3;
    asm("v_pk_fma_f32 %[a0], %[z0], %[za], %[wa]\n\t"
        "v_pk_fma_f32 %[b0], %[z0], %[zb], %[wb]\n\t"
        "v_pk_fma_f32 %[a1], %[z1], %[za], %[wa]\n\t"
        "v_pk_fma_f32 %[b1], %[z1], %[zb], %[wb]\n\t"
        "v_pk_fma_f32 %[a2], %[z2], %[za], %[wa]\n\t"
        "v_pk_fma_f32 %[b2], %[z2], %[zb], %[wb]\n\t"
        "v_pk_fma_f32 %[a3], %[z3], %[za], %[wa]\n\t"
        "v_pk_fma_f32 %[b3], %[z3], %[zb], %[wb]\n\t"
        "v_pk_fma_f32 %[a0], %[y0], %[ya], %[a0]\n\t"
        "v_pk_fma_f32 %[b0], %[y0], %[yb], %[b0]\n\t"
        "v_pk_fma_f32 %[a1], %[y1], %[ya], %[a1]\n\t"
        "v_pk_fma_f32 %[b1], %[y1], %[yb], %[b1]\n\t"
        "v_pk_fma_f32 %[a2], %[y2], %[ya], %[a2]\n\t"
        "v_pk_fma_f32 %[b2], %[y2], %[yb], %[b2]\n\t"
        "v_pk_fma_f32 %[a3], %[y3], %[ya], %[a3]\n\t"
        "v_pk_fma_f32 %[b3], %[y3], %[yb], %[b3]\n\t"
        "v_pk_fma_f32 %[a0], %[x0], %[xa], %[a0]\n\t"
        "v_pk_fma_f32 %[b0], %[x0], %[xb], %[b0]\n\t"
        "v_pk_fma_f32 %[a1], %[x1], %[xa], %[a1]\n\t"
        "v_pk_fma_f32 %[b1], %[x1], %[xb], %[b1]\n\t"
        "v_pk_fma_f32 %[a2], %[x2], %[xa], %[a2]\n\t"
        "v_pk_fma_f32 %[b2], %[x2], %[xb], %[b2]\n\t"
        "v_pk_fma_f32 %[a3], %[x3], %[xa], %[a3]\n\t"
        "v_pk_fma_f32 %[b3], %[x3], %[xb], %[b3]"
        : [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3), [b0] "=&v"(b0), [b1] "=&v"(b1),
          [b2] "=&v"(b2), [b3] "=&v"(b3)
        : [x0] "v"(px[0]), [x1] "v"(px[1]), [x2] "v"(px[2]), [x3] "v"(px[3]), [y0] "v"(py[0]), [y1] "v"(py[1]),
          [y2] "v"(py[2]), [y3] "v"(py[3]), [z0] "v"(pz[0]), [z1] "v"(pz[1]), [z2] "v"(pz[2]), [z3] "v"(pz[3]),
          [xa] "v"(xa), [xb] "v"(xb), [ya] "v"(ya), [yb] "v"(yb), [za] "v"(za), [zb] "v"(zb), [wa] "v"(wa),
          [wb] "v"(wb));
    mn[0] = __builtin_fminf(__builtin_fminf(mn[0], a0.x), a0.y);
    mn[1] = __builtin_fminf(__builtin_fminf(mn[1], a1.x), a1.y);
    mn[2] = __builtin_fminf(__builtin_fminf(mn[2], a2.x), a2.y);
    mn[3] = __builtin_fminf(__builtin_fminf(mn[3], a3.x), a3.y);
    mn[0] = __builtin_fminf(__builtin_fminf(mn[0], b0.x), b0.y);
    mn[1] = __builtin_fminf(__builtin_fminf(mn[1], b1.x), b1.y);
    mn[2] = __builtin_fminf(__builtin_fminf(mn[2], b2.x), b2.y);
    mn[3] = __builtin_fminf(__builtin_fminf(mn[3], b3.x), b3.y);
}

// One workgroup's share of the forward: queries [qbase, qbase + 64 QPT) of
// cloud Q (nq points) against the nt points of T.  Writes D[q], I[q]; returns
// the distance of query slot threadIdx.x (0 past nq and for threads >= 64 QPT),
// for the loss partial.  `arena` holds FiltLds<W, QPT, TILE>::kBytes.
// kSplit: each tile is staged and scanned in parts of NT points (one per
// staged point of a thread), each behind its own barrier, so the scan of the
// first part overlaps the rest of the prologue's load burst.  Chunks are
// visited in the same order (c = wave, wave + W, ...), so results are
// identical.
template <typename TIn, int W, int QPT, int C, int TILE, bool kSc1, bool kSplit = false>
__device__ __forceinline__ float filt_forward(const TIn *__restrict__ Q, const TIn *__restrict__ T, int nq, int nt, int qbase,
                              float *__restrict__ D, int32_t *__restrict__ I, unsigned char *arena,
                              unsigned long long *__restrict__ Gr = nullptr, unsigned long long tag = 0,
                              const PreDma *pre = nullptr, pcm_f4 *qown = nullptr, PcmLay LQ = PcmLay{3, 1},
                              PcmLay LT = PcmLay{3, 1}, unsigned *__restrict__ Gr4 = nullptr, unsigned gtag4 = 0,
                              int *kown = nullptr, bool g4x = false) {
    static_assert(C % 4 == 0 && TILE % C == 0, "tile must hold whole chunks of 4-candidate groups");
    constexpr int QW = 64 * QPT;
    constexpr int NT = 64 * W;
    static_assert(NT >= QW, "one thread per query slot in the merge");
    static_assert(TILE % NT == 0, "whole points per thread when staging");
    constexpr int PARTS = NT / QW;
    constexpr int CP = C / PARTS;
    static_assert(C % PARTS == 0, "chunk must split evenly");
    constexpr int kPer = TILE / NT;  // staged points per thread per tile
    constexpr int kTB = 4;           // near-tie queries per cooperative pass
    float(*sU)[TILE] = reinterpret_cast<float(*)[TILE]>(arena);  // ux, uy, uz, w (SoA)
    // raw (x, y, z, 0) per point after the scan: one ds_read_b128 per candidate
    pcm_f4 *sT = reinterpret_cast<pcm_f4 *>(arena);
    float(*sBest)[QW] = reinterpret_cast<float(*)[QW]>(arena + 4 * TILE * 4);
    float(*sSec)[QW] = reinterpret_cast<float(*)[QW]>(arena + 4 * TILE * 4 + W * QW * 4);
    int(*sChunk)[QW] = reinterpret_cast<int(*)[QW]>(arena + 4 * TILE * 4 + 2 * W * QW * 4);
    __shared__ float sD[QW];  // final (distance, index) per query slot
    __shared__ int sK[QW];
    __shared__ unsigned sPlan[QW];  // near-tie: chunks that can hold the answer (below)
    __shared__ float sTD[kTB * W];  // near-tie pass: per-wave partials
    __shared__ int sTK[kTB * W];
    __shared__ float sHD[PARTS][QW];
    __shared__ int sHK[PARTS][QW];
    __shared__ float sRmax[16];
    __shared__ int sList[QW];
    __shared__ int sNList;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto slot = [](int p) { return filt_slot<C>(p); };  // raw-tile slot of point p

    // ---- queries (every wave holds the same QW queries: lane + 64 qq)
    float rx[QPT], ry[QPT], rz[QPT];
    bool nonfinite = false;
    float cx = 0.f, cy = 0.f, cz = 0.f;
    int qcnt = 0;
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        // unconditional (clamped) loads: every load of the prologue -- these and
        // the first tile's -- is in flight at once (a branch around a load makes
        // hipcc wait for it inside the branch)
        const int qc = min(qbase + qq * 64 + lane, nq - 1);
        rx[qq] = pcm_ld(Q + pcm_at(LQ, qc, 0));
        ry[qq] = pcm_ld(Q + pcm_at(LQ, qc, 1));
        rz[qq] = pcm_ld(Q + pcm_at(LQ, qc, 2));
    }

    float tv[kPer][3];
    auto load_tile = [&](int t0) {
        const int last = min(TILE, nt - t0) - 1;
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const int p = min(tid + r * NT, last);
#pragma unroll
            for (int d = 0; d < 3; ++d) tv[r][d] = pcm_ld(T + pcm_at(LT, t0 + p, d));
        }
    };
    load_tile(0);

#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        if (qbase + qq * 64 + lane < nq) {
            nonfinite |= !(pcm_finite(rx[qq]) && pcm_finite(ry[qq]) && pcm_finite(rz[qq]));
            cx += rx[qq];
            cy += ry[qq];
            cz += rz[qq];
            ++qcnt;
        }
    }

    if (tid == 0) sNList = 0;  // first read after the staging barrier
    // every wave holds the same queries, so each reduces them itself (the
    // same instructions give the same bits): no LDS round trip, no barrier
    const float cn = (float)wave_sum_dpp(qcnt);
    const float c0 = wave_sum_dpp(cx) / cn, c1 = wave_sum_dpp(cy) / cn, c2 = wave_sum_dpp(cz) / cn;
    PCM_STAMP(1);
    if (qown != nullptr && wave < QPT) {
        // the workgroup's own query coordinates, for the caller's gradient
        // phase (wave w writes its register copy w: query slots 64 w + lane)
        float x = rx[0], y = ry[0], z = rz[0];
#pragma unroll
        for (int qq = 1; qq < QPT; ++qq)
            if (qq == wave) { x = rx[qq]; y = ry[qq]; z = rz[qq]; }
        qown[wave * 64 + lane] = pcm_f4{x, y, z, 0.f};
    }

    // centred queries, splatted for the packed math
    pcm_f2 px[QPT], py[QPT], pz[QPT];
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        const float x = rx[qq] - c0, y = ry[qq] - c1, z = rz[qq] - c2;
        px[qq] = pcm_f2{x, x};
        py[qq] = pcm_f2{y, y};
        pz[qq] = pcm_f2{z, z};
    }

    float best[QPT], sec[QPT];
    int bchunk[QPT];
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) { best[qq] = PCM_INF; sec[qq] = PCM_INF; bchunk[qq] = 0; }
    float rt2 = 0.f;  // max |t'|^2 (as computed) over the targets this thread staged

    for (int t0 = 0; t0 < nt; t0 += TILE) {
        const int cnt = min(TILE, nt - t0);
        const int padded = (cnt + C - 1) / C * C;
        if (t0 > 0) {
            load_tile(t0);
            __syncthreads();  // previous tile fully consumed
        }
        constexpr int kParts = kSplit ? kPer : 1;
        constexpr int kRpp = kPer / kParts;  // staged points per thread per part
        static_assert(!kSplit || ((NT % C) == 0 && ((NT / C) % W) == 0), "parts of whole chunks, every wave's share");
#pragma unroll
        for (int h = 0; h < kParts; ++h) {
#pragma unroll
            for (int r = h * kRpp; r < (h + 1) * kRpp; ++r) {
                const int p = tid + r * NT;
                if (p < padded) {
                    float ux = 0.f, uy = 0.f, uz = 0.f, w = PCM_INF;  // pad: a = +inf
                    if (p < cnt) {
                        nonfinite |= !(pcm_finite(tv[r][0]) && pcm_finite(tv[r][1]) && pcm_finite(tv[r][2]));
                        const float x = tv[r][0] - c0, y = tv[r][1] - c1, z = tv[r][2] - c2;
                        w = __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x));
                        rt2 = __builtin_fmaxf(rt2, w);
                        ux = -2.f * x;
                        uy = -2.f * y;
                        uz = -2.f * z;
                    }
                    sU[0][p] = ux;
                    sU[1][p] = uy;
                    sU[2][p] = uz;
                    sU[3][p] = w;
                }
            }
            __syncthreads();
            if (t0 == 0 && h == 0) PCM_STAMP(2);
            if (t0 == 0 && h == 0 && pre) {
                pcm_dma_to_lds(pre->dst1, pre->src1, pre->bytes1, wave, W);
                pcm_dma_to_lds(pre->dst2, pre->src2, pre->bytes2, wave, W);
            }

            // this part's chunks [c_lo, c_hi) (all of the tile's without kSplit)
            const int c_lo = kSplit ? h * kRpp * NT / C : 0;
            const int c_hi = kSplit ? min(padded, (h + 1) * kRpp * NT) / C : padded / C;
            const int gc0 = t0 / C;
            // software-pipelined: the next 4-candidate group's four ds_read_b128
            // are issued before the current group is evaluated (the last group of
            // a chunk prefetches the wave's next chunk, or re-reads this one)
            constexpr int G = C / 4;
            pcm_f4 X4n, Y4n, Z4n, W4n;
            auto fetch = [&](int cc, int g) {
                const int o = cc * C + 4 * g;
                X4n = *reinterpret_cast<const pcm_f4 *>(&sU[0][o]);
                Y4n = *reinterpret_cast<const pcm_f4 *>(&sU[1][o]);
                Z4n = *reinterpret_cast<const pcm_f4 *>(&sU[2][o]);
                W4n = *reinterpret_cast<const pcm_f4 *>(&sU[3][o]);
            };
            if (c_lo + wave < c_hi) fetch(c_lo + wave, 0);
            for (int c = c_lo + wave; c < c_hi; c += W) {
                float mn[QPT];
#pragma unroll
                for (int qq = 0; qq < QPT; ++qq) mn[qq] = PCM_INF;
                const int cn = (c + W < c_hi) ? c + W : c;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const pcm_f4 X4 = X4n, Y4 = Y4n, Z4 = Z4n, W4 = W4n;
                    if (g + 1 < G) fetch(c, g + 1);
                    else fetch(cn, 0);
                    // the next group's four reads stay ahead of this group's math
                    // (hipcc otherwise sinks them to their use and waits on each)
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (QPT == 4) {
                        filt_group4(mn, px, py, pz, X4, Y4, Z4, W4);
                        continue;
                    }
#pragma unroll
                    for (int qq = 0; qq < QPT; ++qq) {
                        const pcm_f2 a01 = __builtin_elementwise_fma(
                            px[qq], X4.xy,
                            __builtin_elementwise_fma(py[qq], Y4.xy, __builtin_elementwise_fma(pz[qq], Z4.xy, W4.xy)));
                        const pcm_f2 a23 = __builtin_elementwise_fma(
                            px[qq], X4.zw,
                            __builtin_elementwise_fma(py[qq], Y4.zw, __builtin_elementwise_fma(pz[qq], Z4.zw, W4.zw)));
                        mn[qq] = __builtin_fminf(__builtin_fminf(mn[qq], a01.x), a01.y);
                        mn[qq] = __builtin_fminf(__builtin_fminf(mn[qq], a23.x), a23.y);
                    }
                }
#pragma unroll
                for (int qq = 0; qq < QPT; ++qq) {
                    // best <= sec always: sec' = median(mn, best, sec)
                    sec[qq] = __builtin_amdgcn_fmed3f(mn[qq], best[qq], sec[qq]);
                    if (mn[qq] < best[qq]) { best[qq] = mn[qq]; bchunk[qq] = gc0 + c; }
                }
            }
        }
    }

    // ---- per-wave (best, second, chunk) to LDS (after the scan tile)
    {
        const float v = pcm_wave_max_f32(rt2);  // rt2 >= 0, never NaN
        if (lane == 0) sRmax[wave] = v;
    }
    __syncthreads();  // every wave is done reading sU
    PCM_STAMP(3);
    // a single-tile cloud is still in this thread's registers: park it in LDS
    // (raw coordinates) for the exact rescans
    const bool resident = nt <= TILE;
    if (resident) {
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const int p = tid + r * NT;
            if (p < nt) {
                sT[slot(p)] = pcm_f4{tv[r][0], tv[r][1], tv[r][2], 0.f};
            }
        }
    }
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        sBest[wave][qq * 64 + lane] = best[qq];
        sSec[wave][qq * 64 + lane] = sec[qq];
        sChunk[wave][qq * 64 + lane] = bchunk[qq];
    }
    __shared__ int sNF[W];
    const int any_nonfinite = pcm_wg_or(nonfinite, sNF, W);
    PCM_STAMP(4);

    float my_d = 0.f;
    if (!any_nonfinite) {
        // ---- one pass, one barrier: thread (s = tid mod QW, part = tid / QW)
        // merges the waves' (best, second, chunk) of query s -- every part
        // reaches the same verdict -- and, when the best chunk is proven,
        // rescans its part of that chunk exactly; part 0 of a near-tie query
        // lists it with its rescan plan instead.
        const int s = tid % QW;
        const int part = tid / QW;
        bool proven = false;
        {
            float vb[W], vs[W], vr[W];
            int vc[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {  // every load first, then branch-free selects
                vb[w] = sBest[w][s];
                vs[w] = sSec[w][s];
                vc[w] = sChunk[w][s];
                vr[w] = sRmax[w];  // with the rest, not one LDS round trip later
            }
            __builtin_amdgcn_sched_barrier(0);
            float fb = vb[0], fs = vs[0];
            int fc = vc[0];
#pragma unroll
            for (int w = 1; w < W; ++w) {
                const bool better = (vb[w] < fb) | ((vb[w] == fb) & (vc[w] < fc));
                fs = __builtin_fminf(__builtin_fminf(fs, vs[w]), better ? fb : vb[w]);
                fb = better ? vb[w] : fb;
                fc = better ? vc[w] : fc;
            }
            float rmax2 = vr[0];
#pragma unroll
            for (int w = 1; w < W; ++w) rmax2 = __builtin_fmaxf(rmax2, vr[w]);
            // this thread's register copy of query s is qq = s >> 6
            const int qsel = s >> 6;
            float qn2 = 0.f, x = rx[0], y = ry[0], z = rz[0];
#pragma unroll
            for (int qq = 0; qq < QPT; ++qq)
                if (qq == qsel) {
                    qn2 = __builtin_fmaf(pz[qq].x, pz[qq].x, __builtin_fmaf(py[qq].x, py[qq].x, px[qq].x * px[qq].x));
                    x = rx[qq];
                    y = ry[qq];
                    z = rz[qq];
                }
            // the bound E = 16u (|t'| + |q'|)^2 of a target t: with R = max |t'|
            // (eR) for every target; but a target that can reach the best
            // chunk's exact minimum d_b lies within sqrt(d_b) of q, so
            // |t'| <= |q'| + sqrt(d_b), and d_b <= fb + |q'|^2 + eR (= db,
            // rounded up): for every target that matters -- the best chunk's
            // argmin included -- E <= 16u (2|q'| + sqrt(db))^2.  If the
            // other chunks' best exceeds fb by twice the smaller bound, no
            // target outside the best chunk can reach d_b (the ICP screen's
            // argument, csrc/icp.hip).  Near ties: 0.12 % of random queries
            // with eR alone.
            // (v_sqrt_f32: within 1 ulp, far inside the 1.001 margins; the
            // correctly rounded sqrtf is a dozen instructions more per root)
            const float sq = __builtin_amdgcn_sqrtf(qn2);
            const float rr = __builtin_amdgcn_sqrtf(rmax2) + sq;
            const float eR = kFiltU16 * (rr * rr) * 1.001f;
            const float db = __builtin_fmaxf((fb + qn2) * 1.0001f + 2.f * eR, 0.f);
            const float rq = 2.f * sq + __builtin_amdgcn_sqrtf(db);
            const float e2 = 2.f * kFiltU16 * __builtin_fminf(rr * rr, rq * rq) * 1.001f;
            proven = (fs - fb) > e2;  // false for NaN
#ifdef PCM_PROBE_NO_TIES
            proven = true;  // timing probe only (make variant V=noties): no near-tie pass, results may differ
#endif
            float hd = PCM_INF;
            int hk = 0x7fffffff;
            if (qbase + s < nq) {
                if (proven) {
                    const int k0 = fc * C + part * CP;
                    float tx[CP], ty[CP], tz[CP];  // all loads in flight at once
                    if (resident) {
#pragma unroll
                        for (int k = 0; k < CP; ++k) {
                            const int kk = slot(min(k0 + k, nt - 1));
                            const pcm_f4 t4 = sT[kk];
                            tx[k] = t4.x;
                            ty[k] = t4.y;
                            tz[k] = t4.z;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < CP; ++k) {
                            const int kk = min(k0 + k, nt - 1);
                            tx[k] = pcm_ld(T + pcm_at(LT, kk, 0));
                            ty[k] = pcm_ld(T + pcm_at(LT, kk, 1));
                            tz[k] = pcm_ld(T + pcm_at(LT, kk, 2));
                        }
                    }
#pragma unroll
                    for (int k = 0; k < CP; ++k) {  // ascending k: strict '<' keeps the lowest
                        const float d = pcm_sqd(tx[k] - x, ty[k] - y, tz[k] - z);
                        const bool take = (d < hd) & (k0 + k < nt);
                        hd = take ? d : hd;
                        hk = take ? k0 + k : hk;
                    }
                } else if (part == 0) {
                    // near-tie plan: by the same argument only targets screened
                    // at <= fb + e2 can reach d_b, so wave w's chunks are
                    // rescanned all (bit W + w: its second-best chunk
                    // qualifies) or only its best one (bit w), or not at all.
                    // NaN keeps every bit (a full scan).
                    unsigned plan = 0;
                    const float thr = fb + e2;
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        plan |= !(vs[w] > thr) ? (1u << (W + w)) : (!(vb[w] > thr) ? (1u << w) : 0u);
                    sPlan[s] = plan;
                    sList[atomicAdd(&sNList, 1)] = s;
                }
            }
            sHD[part][s] = hd;
            sHK[part][s] = hk;
        }
        __syncthreads();
        PCM_STAMP(5);

        // ---- near-ties.  Resident cloud: one wave per query rescans only the
        // chunks its plan names (usually two: the best and one rival, 2C
        // candidates instead of nt), 64 / C chunks per step, then one wave
        // reduction; no barrier until the output phase.  Otherwise the
        // workgroup cooperates over the whole cloud, kTB queries per pass
        // (one pass over the global candidates serves them all).
        const int nl = sNList;
        if (resident) {
            static_assert(C <= 64 && 64 % C == 0 && 64 % W == 0 && (TILE / C) % W == 0,
                          "whole chunks per step; wave w owns the chunks c = w mod W");
            constexpr int kCps = 64 / C;  // chunks per step
            unsigned long long wpat = 0;  // chunk bits c = 0 mod W of one 64-chunk word
#pragma unroll
            for (int i = 0; i < 64; i += W) wpat |= 1ull << i;
            const int nch = (nt + C - 1) / C;
            for (int e = wave; e < nl; e += W) {
                const int s = __builtin_amdgcn_readfirstlane(sList[e]);
                const unsigned plan = __builtin_amdgcn_readfirstlane(sPlan[s]);
                int one[W];  // best chunk of each wave
#pragma unroll
                for (int w = 0; w < W; ++w) one[w] = __builtin_amdgcn_readfirstlane(sChunk[w][s]);
                float x = rx[0], y = ry[0], z = rz[0];
#pragma unroll
                for (int qq = 1; qq < QPT; ++qq)
                    if ((s >> 6) == qq) { x = rx[qq]; y = ry[qq]; z = rz[qq]; }
                // s is wave-uniform: v_readlane, not an LDS permute round trip
                x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), s & 63));
                y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), s & 63));
                z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z), s & 63));
                float bd = PCM_INF;
                int bk = 0x7fffffff;
                for (int c0 = 0; c0 < nch; c0 += 64) {
                    unsigned long long M = 0;
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        if ((plan >> (W + w)) & 1u) M |= wpat << w;
                        else if (((plan >> w) & 1u) && one[w] >= c0 && one[w] < c0 + 64) M |= 1ull << (one[w] - c0);
                    }
                    if (nch - c0 < 64) M &= (1ull << (nch - c0)) - 1ull;
                    while (M) {
                        int ch[kCps];
#pragma unroll
                        for (int j = 0; j < kCps; ++j) {
                            ch[j] = M ? c0 + __builtin_ctzll(M) : -1;
                            M &= M - 1ull;
                        }
                        int c = ch[0];
#pragma unroll
                        for (int j = 1; j < kCps; ++j)
                            if (lane / C == j) c = ch[j];
                        const int k = c * C + (lane & (C - 1));
                        const int sk = slot(min(max(k, 0), nt - 1));
                        const pcm_f4 t4 = sT[sk];
                        const float d = pcm_sqd(t4.x - x, t4.y - y, t4.z - z);
                        if (c >= 0 && k < nt) pcm_lexmin(bd, bk, d, k);
                    }
                }
                pcm_wave_lexmin(bd, bk);
                if (lane == 0) {
                    sD[s] = bd;
                    sK[s] = bk;
                }
            }
            if (nl > 0) __syncthreads();
        }
        for (int e0 = 0; e0 < (resident ? 0 : nl); e0 += kTB) {
            float qx[kTB], qy[kTB], qz[kTB], bd[kTB];
            int bk[kTB];
#pragma unroll
            for (int j = 0; j < kTB; ++j) {
                // query slot s lives in register copy s >> 6 of lane s & 63
                // (every wave holds every query): broadcast it with ds_bpermute
                const int s = sList[min(e0 + j, nl - 1)];
                float x = rx[0], y = ry[0], z = rz[0];
#pragma unroll
                for (int qq = 1; qq < QPT; ++qq)
                    if ((s >> 6) == qq) { x = rx[qq]; y = ry[qq]; z = rz[qq]; }
                qx[j] = __shfl(x, s & 63, 64);
                qy[j] = __shfl(y, s & 63, 64);
                qz[j] = __shfl(z, s & 63, 64);
                bd[j] = PCM_INF;
                bk[j] = 0x7fffffff;
            }
            auto visit = [&](int k, float x, float y, float z) {
#pragma unroll
                for (int j = 0; j < kTB; ++j) {
                    const float d = pcm_sqd(x - qx[j], y - qy[j], z - qz[j]);
                    pcm_lexmin(bd[j], bk[j], d, k);
                }
            };
            {
                constexpr int U = 8;  // candidates per thread with loads in flight together
                for (int k0 = tid; k0 < nt; k0 += U * NT) {
                    float tx[U], ty[U], tz[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int k = min(k0 + u * NT, nt - 1);
                        tx[u] = pcm_ld(T + pcm_at(LT, k, 0));
                        ty[u] = pcm_ld(T + pcm_at(LT, k, 1));
                        tz[u] = pcm_ld(T + pcm_at(LT, k, 2));
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (k0 + u * NT < nt) visit(k0 + u * NT, tx[u], ty[u], tz[u]);
                }
            }
#pragma unroll
            for (int j = 0; j < kTB; ++j) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float od = __shfl_xor(bd[j], o, 64);
                    const int ok = __shfl_xor(bk[j], o, 64);
                    pcm_lexmin(bd[j], bk[j], od, ok);
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < kTB; ++j) {
                    sTD[j * W + wave] = bd[j];
                    sTK[j * W + wave] = bk[j];
                }
            }
            __syncthreads();
            if (tid < kTB && e0 + tid < nl) {
                float d = sTD[tid * W];
                int k = sTK[tid * W];
                for (int w = 1; w < W; ++w) {
                    const float dv = sTD[tid * W + w];
                    const int kv = sTK[tid * W + w];
                    pcm_lexmin(d, k, dv, kv);
                }
                const int s = sList[e0 + tid];
                sD[s] = d;
                sK[s] = k;
            }
            __syncthreads();
        }
        PCM_STAMP(6);
        // ---- one store phase for the workgroup's outputs (thread tid < QW is
        // part 0 of query tid: `proven` is that query's verdict)
        int kg = 0;  // this thread's argmin, for the 16-byte granule stores
        if (tid < QW && qbase + tid < nq) {
            float d;
            int k;
            if (proven) {
                d = sHD[0][tid];
                k = sHK[0][tid];
#pragma unroll
                for (int p = 1; p < PARTS; ++p) pcm_lexmin(d, k, sHD[p][tid], sHK[p][tid]);
            } else {
                d = sD[tid];
                k = sK[tid];
            }
            my_d = d;
            out_st<kSc1>(D + qbase + tid, d);
            out_st<kSc1>(I + qbase + tid, (int32_t)k);
            // data-tagged argmin granule {call tag, idx}: one 8-byte sc1 store,
            // its own flag (no drain, no counter)
            if (Gr) __hip_atomic_store(Gr + qbase + tid, tag | (unsigned)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // 4-byte granule {tag << 11 | idx} (chamfer_lgrid.h's format)
            if (Gr4 && !g4x)
                __hip_atomic_store(Gr4 + qbase + tid, gtag4 | (unsigned)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (kown) *kown = k;
            kg = k;
        }
        if (Gr4 && g4x && tid < QW) {
            // g4x: four consecutive queries' granules per 16-byte sc1 store
            // (lanes 0-15 of each query wave gather them from lanes 4L..4L+3):
            // a write-through store costs per lane, so a quarter of the
            // fabric writes (MI355X_MICROARCH.md store table).  Every 4-byte
            // granule carries its own tag, so a torn 16-byte store is harmless.
            const unsigned v = gtag4 | (unsigned)kg;
            const int src = (lane & 15) * 4;
            pcm_u32x4 g;
            g.x = (unsigned)__shfl((int)v, src, 64);
            g.y = (unsigned)__shfl((int)v, src + 1, 64);
            g.z = (unsigned)__shfl((int)v, src + 2, 64);
            g.w = (unsigned)__shfl((int)v, src + 3, 64);
            const int q = qbase + (tid & ~63) + src;
            if (lane < 16 && q < nq) {
                if (q + 3 < nq) {
                    pcm_st_sc1_x4(Gr4 + q, g);
                } else {
                    __hip_atomic_store(Gr4 + q, g.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (q + 1 < nq) __hip_atomic_store(Gr4 + q + 1, g.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (q + 2 < nq) __hip_atomic_store(Gr4 + q + 2, g.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    } else {
        for (int s = tid; s < QW; s += NT) {
            const int qi = qbase + s;
            if (qi >= nq) continue;
            float d;
            int idx;
            pcm_ref_nn_scan(pcm_ld(Q + pcm_at(LQ, qi, 0)), pcm_ld(Q + pcm_at(LQ, qi, 1)),
                            pcm_ld(Q + pcm_at(LQ, qi, 2)), T, nt, d, idx, LT);
            my_d = d;
            out_st<kSc1>(D + qi, d);
            out_st<kSc1>(I + qi, (int32_t)idx);
            if (Gr) __hip_atomic_store(Gr + qi, tag | (unsigned)idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (Gr4) __hip_atomic_store(Gr4 + qi, gtag4 | (unsigned)idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (kown) *kown = idx;
        }
    }
    return my_d;
}

// ---------------------------------------------------------------------------
// Filtered forward on the matrix cores (single-tile clouds, nt <= 1024; 8
// waves, 256 queries).  Same contract and results as filt_forward.
//
// The screen value a(q, t) = w + u.q' (u = -2t', w = |t'|^2 as filt_forward
// computes them) is evaluated by v_mfma_f32_16x16x32_bf16 on a three-way
// bf16 split of every operand: v = vh + vm + vl + e, |e| <= 2^-24 |v| (each
// part the round-to-nearest bf16 of the remainder, remainders exact in fp32).
// Per dimension the K axis carries uh.qh, uh.qm, um.qh, uh.ql, ul.qh, um.qm
// (dropped: um.ql, ul.qm, ul.ql, each <= 2^-24 |u_d q_d|), then wh, wm, wl
// against 1: 21 of the 32 K slots, products exact in fp32.  Error of the
// screened value against the real w + u.q':
//   split and dropped terms   <= 4.01 u |u||q| + u w <= 4.01 u (R + |q'|)^2
//   20 fp32 additions, any order, rounding or truncating (2u each)
//                              <= 40 u * 1.02 (w + |u||q|) <= 41 u (R + |q'|)^2
// plus filt_forward's own terms (w 2u, centring 2u, the exact formula 5u,
// slack): 59 u; the proof uses E = 80 u (R + |q'|)^2 (kFiltU80) and an
// absolute 2^-100 for subnormal parts.
//
// MFMA roles: A = 16 targets x 32 K (rows), B = 32 K x 16 queries (columns),
// so lane l receives D[targets 4(l>>4)..+3][query l&15] -- four candidates of
// ONE query, folded with two v_min3 and no cross-lane work.  Wave (quarter,
// half): queries of half h (8 tiles of 16), target groups of 64 (4 tiles)
// g = quarter, quarter + 4, ...  A chunk (the unit of the proof) is one
// target group seen by one lane group: targets 64 g + 16 i + 4 (l>>4) + r,
// i, r in 0..3 -- 16 candidates, rescanned in ascending order.
//
// Around the screen the forward is filt_forward's: no barrier before staging
// (every wave loads the 256 queries and reduces the centre itself), the next
// group's A tiles read a group ahead, the lane groups folded in registers,
// the merge of the four quarters, the proof and the exact rescan in one pass
// by (query, part) threads, near ties rescanned over their plan's chunks only
// by the two waves that hold the query (no list, no second barrier: the
// query, its plan and its chunks come from registers by v_readlane, and a
// wave's near ties alternate between the two parts), and the per-query bound: E above
// with (R + |q'|)^2 replaced by min((R + |q'|)^2, (2|q'| + sqrt(d_b))^2), by
// filt_forward's argument.  Fused variants 6 and 19.
//
// The wide form (kWide; the one-launch step's default, fused variant 20) runs
// the same screen on v_mfma_f32_32x32x16_bf16: an MFMA holds its SIMD's vector
// issue for 8 cycles whatever its shape, so 1024 values per instruction
// instead of 256 halve the MFMA issue slots of the loop, which is bound by
// vector issue, not by the matrix pipe.  Staging, the LDS image, the arena and
// the proof are the narrow form's.  A = 32 targets x 16 K, B = 16 K x 32
// queries, two chained MFMAs per (A tile, query tile): K 0..15 onto an inline
// zero, then K 16..31 onto that result in place.  Lane l receives
// D[targets 8 j + 4 (l >> 5) + r][query l & 31] in element 4 j + r: sixteen
// candidates of ONE query, folded with eight v_min3 and no cross-lane work.
// Wave (quarter, half): the half's 128 queries are four tiles of 32 (their
// eight B operands stay in registers), a 64-target group is two A tiles.  A
// chunk is one A tile seen by one lane half -- targets
// 64 g + 32 i + 8 j + 4 h + r, id 4 g + 2 i + h -- still 16 candidates, 64 ids
// per 1024 targets and four chunks per quarter and group, so the merge, the
// proof and the plans are unchanged; only the maps from a chunk id to its
// candidates (exact rescan, near-tie single-chunk step) differ.
// The error bound is unchanged: the 21 live K slots are K 0..15 in the first
// MFMA and K 16..20 in the second, their products are the same exact ones,
// adding the zero C is exact, and the 20 fp32 additions "in any order,
// rounding or truncating" are the same 20 (tests/test_mfma_wide_bound_cpu.py
// restates them in several orders).  Pad rows (wh = +inf at K 18) and an
// overflowed w screen as in the narrow form.
// ---------------------------------------------------------------------------
constexpr float kFiltU80 = 4.76837158203125e-06f;  // 80 u = 80 * 2^-24
constexpr int kMfmaQW = 256, kMfmaNT = 512, kMfmaTile = 1024;
// Operand rows in LDS: 768 bytes per 16-row MFMA tile, K-slice-major inside
// the tile -- 16 bytes (K 8j..8j+7, j = 0..2) of row 16 t + c at uint4 index
// 48 t + 16 j + c -- so lane groups 0-2 read a tile as lane l's uint4 48 t + l
// (consecutive bytes) and a wave's row store covers consecutive 256-byte runs
// (row-major 64-byte rows put every fourth lane of a store on the same banks:
// staging took 2.4 us that way, profiles/mfma_screen).  K 24..31 are zero in
// every row of both operands: lane group 3 reads them from a zero region that
// spans the four tile offsets of a group.  With the zero slices stored the
// arena would exceed the gradient phase's 64 KiB and the grid's polling
// workgroup would no longer be resident beside a CU's forward workgroup.
struct MfmaLds {
    static constexpr int kA = kMfmaTile * 48;                    // target rows, K 0..23
    static constexpr int kZ = (3 * 48 + 16) * 16;                // zeros: tile offsets 0, 48, 96, 144 (+ 16 columns)
    static constexpr int kQB = kMfmaQW * 48;                     // query rows, K 0..23
    static constexpr int kScan = kA + kZ + kQB;
    static constexpr int kTail = 3 * kMfmaTile * 4 + 3 * 4 * kMfmaQW * 4;  // raw tile + 4 partials
    static constexpr int kBytes = kScan > kTail ? kScan : kTail;
};
typedef __bf16 pcm_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pcm_f16v __attribute__((ext_vector_type(16)));  // a 32 x 32 MFMA result: 16 rows of the lane's column

typedef __bf16 pcm_bf16x2 __attribute__((ext_vector_type(2)));
// (a, b) -> one dword of two round-to-nearest-even bf16 (v_cvt_pk_bf16_f32): a low, b high
__device__ __forceinline__ unsigned cvt_bf16x2(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((pcm_f2){a, b}, pcm_bf16x2));
}
__device__ __forceinline__ float bf_lo(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bf_hi(unsigned v) { return __uint_as_float(v & 0xffff0000u); }
// dword from the 16-bit halves: low half of `lo` word (hl = 0) or its high half (hl = 1), etc.
template <int HL, int HH>
__device__ __forceinline__ unsigned bf_pair(unsigned lo, unsigned hi) {
    constexpr unsigned sel = (HL ? 0x0302u : 0x0100u) | ((HH ? 0x0706u : 0x0504u) << 16);
    return __builtin_amdgcn_perm(hi, lo, sel);
}
// Three-way bf16 split of (a, b): a = lo16 parts of H, M, L; b = the high parts.
// Each level is the RNE bf16 of the remainder of the levels above; every
// remainder is exact in fp32.
[[maybe_unused]] __device__ __forceinline__ void split3x2(float a, float b, unsigned &H, unsigned &M, unsigned &L) {
    H = cvt_bf16x2(a, b);
    const float ra = a - bf_lo(H), rb = b - bf_hi(H);
    M = cvt_bf16x2(ra, rb);
    L = cvt_bf16x2(ra - bf_lo(M), rb - bf_hi(M));
}
// 64-target groups of the raw tile rotated by 4 (group mod 8): the rescan's
// lanes -- one query each, chunks of stride-16 quads -- spread over the banks
[[maybe_unused]] __device__ __forceinline__ int mslot(int p) { return (p & ~63) | ((p + 4 * ((p >> 6) & 7)) & 63); }

// One halving step of the fold over a wave's four lane groups, which hold
// partials (best, second, chunk) of the same queries.  Lanes l and l ^ 32
// (k32; else l ^ 16) hold partials X of query A and Y of query B.
// v_permlane32/16_swap exchanges X of the upper lane with Y of the lower one,
// so the lower lane ends with both partials of A and the upper lane with both
// of B: each folds the query it keeps into X, and the step halves the queries
// a lane carries.  The fold is symmetric.  No LDS round trip.
template <bool k32>
__device__ __forceinline__ void mfma_fold_step(float &b, float &s, int &c, float bo, float so, int co) {
    auto swap = [](unsigned &x, unsigned &y) {
        if constexpr (k32) {
            const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
            x = r[0];
            y = r[1];
        } else {
            const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
            x = r[0];
            y = r[1];
        }
    };
    unsigned b0 = __float_as_uint(b), b1 = __float_as_uint(bo), s0 = __float_as_uint(s), s1 = __float_as_uint(so);
    unsigned c0 = (unsigned)c, c1 = (unsigned)co;
    swap(b0, b1);
    swap(s0, s1);
    swap(c0, c1);
    const float fb0 = __uint_as_float(b0), fb1 = __uint_as_float(b1);
    const bool better = (fb1 < fb0) | ((fb1 == fb0) & ((int)c1 < (int)c0));
    s = __builtin_fminf(__builtin_fminf(__uint_as_float(s0), __uint_as_float(s1)), better ? fb0 : fb1);
    b = better ? fb1 : fb0;
    c = better ? (int)c1 : (int)c0;
}

// Gr / tag: the argmin granules of the one-launch step's hand-off (as
// filt_forward publishes them); kown: the thread's own argmin; LQ / LT: the
// clouds' layouts (prologue loads only: everything after works on registers
// and LDS).
template <bool kSc1, bool kWide = false>
__device__ __forceinline__ float filt_forward_mfma(const float *__restrict__ Q, const float *__restrict__ T, int nq,
                                                   int nt, int qbase, float *__restrict__ D, int32_t *__restrict__ I,
                                                   unsigned char *arena, unsigned long long *__restrict__ Gr = nullptr,
                                                   unsigned long long tag = 0, PcmLay LQ = PcmLay{3, 1},
                                                   PcmLay LT = PcmLay{3, 1}, int *kown = nullptr) {
    constexpr int QW = kMfmaQW, NT = kMfmaNT, W = NT / 64, TILE = kMfmaTile, QPT = QW / 64;
    constexpr int kPer = TILE / NT;  // staged targets per thread
    static_assert(NT == 2 * QW && QPT == 4, "thread = (query slot, part of 2); wave w holds query copy w mod 4");
    uint4 *sA = reinterpret_cast<uint4 *>(arena);                                   // [TILE / 16][3][16] x 16 B
    uint4 *sZ = reinterpret_cast<uint4 *>(arena + MfmaLds::kA);                     // zeros
    uint4 *sQB = reinterpret_cast<uint4 *>(arena + MfmaLds::kA + MfmaLds::kZ);      // [QW / 16][3][16]
    auto rowslot = [](int p, int j) { return 48 * (p >> 4) + 16 * j + (p & 15); };  // K slice j < 3 of row p
    float(*sT)[TILE] = reinterpret_cast<float(*)[TILE]>(arena);         // raw x, y, z (after the scan)
    float(*sPB)[QW] = reinterpret_cast<float(*)[QW]>(arena + 3 * TILE * 4);
    float(*sPS)[QW] = reinterpret_cast<float(*)[QW]>(arena + 3 * TILE * 4 + 4 * QW * 4);
    int(*sPC)[QW] = reinterpret_cast<int(*)[QW]>(arena + 3 * TILE * 4 + 8 * QW * 4);
    __shared__ float sHD[2][QW];  // each part's exact (distance, index) of the query
    __shared__ int sHK[2][QW];
    __shared__ float sRmax[W];
    __shared__ int sNFm[W];
#ifdef PCM_STAMPS
    __shared__ unsigned sCensus[4];  // near ties, whole quarters, single chunks, most iterations of a wave
    if (threadIdx.x < 4) sCensus[threadIdx.x] = 0;  // first touched after the staging barrier
#endif

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- queries (every wave holds the same QW queries: lane + 64 qq) and
    // this thread's targets: unconditional clamped loads, all in flight at once
    float rx[QPT], ry[QPT], rz[QPT];
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        const int qc = min(qbase + qq * 64 + lane, nq - 1);
        rx[qq] = pcm_ld(Q + pcm_at(LQ, qc, 0));
        ry[qq] = pcm_ld(Q + pcm_at(LQ, qc, 1));
        rz[qq] = pcm_ld(Q + pcm_at(LQ, qc, 2));
    }
    float tv[kPer][3];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int p = min(tid + r * NT, nt - 1);
#pragma unroll
        for (int d = 0; d < 3; ++d) tv[r][d] = pcm_ld(T + pcm_at(LT, p, d));
    }
    bool nonfinite = false;
    float cx = 0.f, cy = 0.f, cz = 0.f;
    int qcnt = 0;
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        if (qbase + qq * 64 + lane < nq) {
            nonfinite |= !(pcm_finite(rx[qq]) && pcm_finite(ry[qq]) && pcm_finite(rz[qq]));
            cx += rx[qq];
            cy += ry[qq];
            cz += rz[qq];
            ++qcnt;
        }
    }
    // every wave reduces the centre itself (same instructions, same bits): no barrier
    const float cn = (float)wave_sum_dpp(qcnt);
    const float c0 = wave_sum_dpp(cx) / cn, c1 = wave_sum_dpp(cy) / cn, c2 = wave_sum_dpp(cz) / cn;
    PCM_STAMP(1);
#ifdef PCM_STAMPS
    if (tid == 0 && blockIdx.x < 4096)  // shader-clock cycles beside the 100 MHz stamps (clock estimate)
        g_pcm_stamps[(8192 + blockIdx.x) * 8 + 1] = __builtin_amdgcn_s_memtime();
#endif

    // ---- this thread's query: slot s = tid mod QW is register copy wave mod 4
    // of its lane.  It splits that query's row (waves 0-3 store the row's first
    // half, waves 4-7 the second) and later proves and rescans it as part
    // tid / QW.
    float qx = rx[0], qy = ry[0], qz = rz[0];
#pragma unroll
    for (int qq = 1; qq < QPT; ++qq)
        if ((wave & (QPT - 1)) == qq) { qx = rx[qq]; qy = ry[qq]; qz = rz[qq]; }
    const float qxc = qx - c0, qyc = qy - c1, qzc = qz - c2;
    {
        unsigned H01, M01, L01, H2, M2, L2;
        split3x2(qxc, qyc, H01, M01, L01);
        split3x2(qzc, 0.f, H2, M2, L2);
        // K 6d..6d+5: qh, qm, qh, ql, qh, qm; K 18..20: 1
        const unsigned one2 = 0x3f803f80u, one0 = 0x00003f80u;
        const int row = tid & (QW - 1);
        if (wave < QPT) {
            sQB[rowslot(row, 0)] = make_uint4(bf_pair<0, 0>(H01, M01), bf_pair<0, 0>(H01, L01), bf_pair<0, 0>(H01, M01),
                                              bf_pair<1, 1>(H01, M01));
            sQB[rowslot(row, 1)] = make_uint4(bf_pair<1, 1>(H01, L01), bf_pair<1, 1>(H01, M01), bf_pair<0, 0>(H2, M2),
                                              bf_pair<0, 0>(H2, L2));
        } else {
            sQB[rowslot(row, 2)] = make_uint4(bf_pair<0, 0>(H2, M2), one2, one0, 0u);
            if (row < MfmaLds::kZ / 16) sZ[row] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    // ---- target rows, 16 dwords each.  The loads were clamped, so a pad row
    // (p >= nt, up to whole 64-target groups) holds a real point until the
    // selects below make it screen as +inf; checking it again is harmless.
    const int ntp = (nt + 63) & ~63;
    float rt2 = 0.f;
    uint4 rows[kPer][3];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        nonfinite |= !(pcm_finite(tv[r][0]) && pcm_finite(tv[r][1]) && pcm_finite(tv[r][2]));
        const float x = tv[r][0] - c0, y = tv[r][1] - c1, z = tv[r][2] - c2;
        const float w = __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x));
        unsigned H01, M01, L01, H23, M23, L23;
        split3x2(-2.f * x, -2.f * y, H01, M01, L01);
        split3x2(-2.f * z, w, H23, M23, L23);
        // (a w whose high part rounds up to +inf screens as NaN, which the min
        // folds drop: its high part in R makes the bound infinite instead)
        rt2 = __builtin_fmaxf(rt2, __builtin_fmaxf(w, bf_hi(H23)));
        const bool pad = tid + r * NT >= nt;
        // K 6d..6d+5: uh, uh, um, uh, ul, um; K 18..20: wh, wm, wl; pad: K 18 (wh) = +inf, the rest 0
        rows[r][0] = make_uint4(bf_pair<0, 0>(H01, H01), bf_pair<0, 0>(M01, H01), bf_pair<0, 0>(L01, M01),
                                bf_pair<1, 1>(H01, H01));
        rows[r][1] = make_uint4(bf_pair<1, 1>(M01, H01), bf_pair<1, 1>(L01, M01), bf_pair<0, 0>(H23, H23),
                                bf_pair<0, 0>(M23, H23));
        rows[r][2] = make_uint4(bf_pair<0, 0>(L23, M23), bf_pair<1, 1>(H23, M23), L23 >> 16, 0u);
        if (pad) {
            rows[r][0] = make_uint4(0u, 0u, 0u, 0u);
            rows[r][1] = make_uint4(0u, 0u, 0u, 0u);
            rows[r][2] = make_uint4(0u, 0x00007f80u, 0u, 0u);
        }
    }
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int p = tid + r * NT;
        if (p < ntp) {  // a row's 16-byte stores back to back
            sA[rowslot(p, 0)] = rows[r][0];
            sA[rowslot(p, 1)] = rows[r][1];
            sA[rowslot(p, 2)] = rows[r][2];
        }
    }
    {
        const float v = pcm_wave_max_f32(rt2);  // rt2 >= 0, never NaN
        if (lane == 0) sRmax[wave] = v;
    }
    __syncthreads();
    PCM_STAMP(2);
#ifdef PCM_STAMPS
    if (tid == 0 && blockIdx.x < 4096) g_pcm_stamps[(8192 + blockIdx.x) * 8 + 2] = __builtin_amdgcn_s_memtime();
#endif

    // ---- screen: wave (quarter, half); lane group g = lane >> 4 holds K slice 8g..8g+7
    const int quarter = wave >> 1, half = wave & 1;
    const int g = lane >> 4, col = lane & 15;
    constexpr int QT = QW / 2 / 16;  // query tiles per wave
    // lane group 3 (K 24..31) reads zeros whatever the tile: its tile steps are 0
    const uint4 *pq = g < 3 ? sQB + 48 * half * QT + lane : sZ + col;
    const uint4 *pa = g < 3 ? sA + lane : sZ + col;
    const int tstep = g < 3 ? 48 : 0;
    float best[QT], sec[QT];  // (the wide form uses the first QTW of each)
    int bchunk[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { best[qt] = PCM_INF; sec[qt] = PCM_INF; bchunk[qt] = 0; }
    const int ngroups = ntp >> 6;
    // the wide form's lane roles: column (query of a 32-query tile, target row
    // of a 32-row A tile) and K half
    const int wh = lane >> 5, wc = lane & 31;
    constexpr int QTW = QW / 2 / 32;  // 32-query tiles per wave
    // (the wide loop has no register to spare: |q'|^2 crosses it, not q' --
    // the empty asm keeps the compiler from sinking the sum behind the loop)
    float qn2w = kWide ? __builtin_fmaf(qzc, qzc, __builtin_fmaf(qyc, qyc, qxc * qxc)) : 0.f;
    if constexpr (kWide) asm volatile("" : "+v"(qn2w));
    if constexpr (kWide) {
        // ---- the wide screen (header: "The wide form").  Row p's slice j sits at
        // uint4 48 (p >> 4) + 16 j + (p & 15).  The K-low operand of a 32-row
        // tile is lane l's row wc, slice wh (K 8 wh..8 wh + 7).  The K-high
        // MFMA carries slice 2 (K 16..23) in lanes 32-63 and the zero slots
        // (K 24..31) in lanes 0-31: the queries' operand reads those from the
        // zero region, once; the targets' one reads slice wh + 1 in every
        // lane -- slice 1 in lanes 0-31, any finite values against those zeros
        // -- so that a tile's two reads are one address and an immediate.  (A
        // finite coordinate whose doubled bf16 part overflows would put
        // inf x 0 = NaN there: its w is +inf too, R with it, and no screened
        // value is trusted.)  Every 16-lane run of a read is 256 consecutive
        // bytes.
        const int r16 = 48 * (wc >> 4) + (wc & 15);
        const uint4 *pql = sQB + 48 * (QW / 2 / 16) * half + r16 + 16 * wh;
        const uint4 *pqh = wh ? sQB + 48 * (QW / 2 / 16) * half + r16 + 32 : sZ + wc;
        const uint4 *pal = sA + r16 + 16 * wh;
        const int hstep = wh ? 96 : 0;  // the query tiles' K-high step (none inside the zero region)
        pcm_bf16x8 bl[QTW], bh[QTW];
#pragma unroll
        for (int qt = 0; qt < QTW; ++qt) {
            bl[qt] = __builtin_bit_cast(pcm_bf16x8, pql[96 * qt]);
            bh[qt] = __builtin_bit_cast(pcm_bf16x8, pqh[hstep * qt]);
        }
        // the group's two A tiles, K-low and K-high: four ds_read_b128 per
        // group, each re-read in place for the wave's next group right after
        // its last MFMA (the wave's last group re-reads itself)
        uint4 al[2], ah[2];
        auto fetch_lo = [&](int gi, int i) { al[i] = pal[192 * gi + 96 * i]; };
        auto fetch_hi = [&](int gi, int i) { ah[i] = pal[192 * gi + 96 * i + 16]; };
        if (quarter < ngroups) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { fetch_lo(quarter, i); fetch_hi(quarter, i); }
        }
        // A group is eight pairs k = (A tile k / 4, query tile k mod 4) of
        // chained MFMAs -- K 0..15 onto zero, K 16..31 onto that result in
        // place -- over kAcc rotating 32 x 32 results.  Between pair k's two
        // MFMAs stands the best/second/chunk update of pair k - 2, made with
        // the minimum the fold before left: the second MFMA accumulates onto
        // the first one's result and would otherwise wait it out with nothing
        // of its wave to issue (back to back: 49 instead of 44 cycles per 256
        // values).  Behind the second MFMA pair k - 1
        // is folded (sixteen candidates of the lane's query, eight v_min3): a
        // pair, an update and a fold later than its own MFMAs, so no fold waits
        // for its result.  The sequence runs on across the groups: a group's
        // last pair is folded and its last two updated behind the next group's
        // first two (before the wave's first group the results and the minimum
        // hold +inf: those updates change nothing), the wave's last behind the
        // loop.  A query tile's updates stay in A-tile order.  The fences pin
        // this order.
        constexpr int kAcc = 2;
        static_assert(8 % kAcc == 0, "the rotation runs on across the groups");
        pcm_f16v acc[kAcc];
#pragma unroll
        for (int r = 0; r < kAcc; ++r)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[r][e] = PCM_INF;
        float mnw = PCM_INF;  // the minimum of the pair folded last
        // pair k (chunk cid of this lane) updated with mnw.  best is a
        // minimum, not a select on the compare's mask: that mask is then read
        // two instructions after the compare and needs no wait (a NaN mnw --
        // sixteen overflowed w -- leaves best alone either way).  It is
        // written as a v_min3 against +inf, like the fold's first: a
        // two-operand minimum would first canonicalise its operands.
        auto update = [&](int k, int cid) {
            const int qt = k % QTW;
            sec[qt] = __builtin_amdgcn_fmed3f(mnw, best[qt], sec[qt]);
            bchunk[qt] = mnw < best[qt] ? cid : bchunk[qt];
            best[qt] = __builtin_fminf(__builtin_fminf(PCM_INF, mnw), best[qt]);
        };
        auto fold = [&](int k) {  // pair k's sixteen candidates into mnw: eight v_min3
            const pcm_f16v r = acc[k % kAcc];
            mnw = __builtin_fminf(__builtin_fminf(PCM_INF, r[0]), r[1]);
#pragma unroll
            for (int e = 2; e < 16; e += 2) mnw = __builtin_fminf(__builtin_fminf(mnw, r[e]), r[e + 1]);
        };
        pcm_f16v zero16;
#pragma unroll
        for (int e = 0; e < 16; ++e) zero16[e] = 0.f;
        int clast = 0;  // the group before: its last chunk of this lane
        for (int gi = quarter; gi < ngroups; gi += 4) {
            const int gn = gi + 4 < ngroups ? gi + 4 : gi;
            const int cbase = 4 * gi + wh;
#pragma unroll
            for (int k = 0; k < 2 * QTW; ++k) {
                acc[k % kAcc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(pcm_bf16x8, al[k / QTW]),
                                                                        bl[k % QTW], zero16, 0, 0, 0);
                if (k % QTW == QTW - 1) fetch_lo(gn, k / QTW);
                __builtin_amdgcn_sched_barrier(0);
                if (k < 2) update(2 * QTW - 2 + k, clast);
                else update(k - 2, cbase + 2 * ((k - 2) / QTW));
                __builtin_amdgcn_sched_barrier(0);
                acc[k % kAcc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(pcm_bf16x8, ah[k / QTW]),
                                                                        bh[k % QTW], acc[k % kAcc], 0, 0, 0);
                if (k % QTW == QTW - 1) fetch_hi(gn, k / QTW);
                __builtin_amdgcn_sched_barrier(0);
                fold((k + 2 * QTW - 1) % (2 * QTW));
                __builtin_amdgcn_sched_barrier(0);
            }
            clast = cbase + 2;
        }
        update(2 * QTW - 2, clast);
        fold(2 * QTW - 1);
        update(2 * QTW - 1, clast);
    } else {
        pcm_bf16x8 bq[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) bq[qt] = __builtin_bit_cast(pcm_bf16x8, pq[qt * tstep]);
        // software-pipelined: each of the four A tiles (one ds_read_b128 each)
        // is read for the wave's next group while the current group is screened
        // (the wave's last group re-reads itself)
        uint4 an[4];
        // (lane group 3: the tile offset 48 i inside the zero region, no group step)
        auto fetch = [&](int gi, int i) { an[i] = pa[4 * gi * tstep + 48 * i]; };
        if (quarter < ngroups) {
#pragma unroll
            for (int i = 0; i < 4; ++i) fetch(quarter, i);
        }
        // A group's 32 MFMAs (tile i = k / 8 against query tile k mod 8) are one
        // sequence over kRot rotating result quads: MFMA k, then the two folds of
        // MFMA k - kLag, whose result has landed by then, so no MFMA waits for a
        // fold and no fold for its MFMA.  The sequence runs on across the groups:
        // a group's last kLag results are folded behind the next group's first
        // MFMAs (before the wave's first group the quads hold +inf), and the
        // best/second/chunk update of the group before sits in the first eight
        // gaps, behind those folds and ahead of each query tile's first fold of
        // this group (mn = +inf before the first group: that update changes
        // nothing).  The last group's folds and update follow the loop.  A query
        // tile's folds stay in tile order 0..3.  Tile i is re-read in place for
        // the next group right after its eight MFMAs: one read per eight MFMAs,
        // no second buffer and no copy.  A fence behind every MFMA and behind its
        // gap's folds pins this order (left to itself hipcc puts some folds ahead
        // of their gap's MFMA, one instruction short of the result's latency).
        constexpr int kRot = 4, kLag = 3;
        float mn[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) mn[qt] = PCM_INF;
        pcm_f4 d[kRot];
#pragma unroll
        for (int r = 0; r < kRot; ++r) d[r] = pcm_f4{PCM_INF, PCM_INF, PCM_INF, PCM_INF};
        int cid = 0;  // chunk of the group whose mins mn holds
        auto fold = [&](int k, bool first) {  // (a group's first fold of a query tile starts from +inf)
            const pcm_f4 r = d[k % kRot];
            mn[k % QT] = __builtin_fminf(__builtin_fminf(first ? PCM_INF : mn[k % QT], r.x), r.y);
            mn[k % QT] = __builtin_fminf(__builtin_fminf(mn[k % QT], r.z), r.w);
        };
        auto update = [&](int qt) {
            sec[qt] = __builtin_amdgcn_fmed3f(mn[qt], best[qt], sec[qt]);
            if (mn[qt] < best[qt]) { best[qt] = mn[qt]; bchunk[qt] = cid; }
        };
        for (int gi = quarter; gi < ngroups; gi += 4) {
            const int gn = gi + 4 < ngroups ? gi + 4 : gi;
#pragma unroll
            for (int k = 0; k < 4 * QT; ++k) {
                d[k % kRot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(pcm_bf16x8, an[k / QT]), bq[k % QT], pcm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                if (k % QT == QT - 1) fetch(gn, k / QT);
                __builtin_amdgcn_sched_barrier(0);
                if (k < kLag) fold(4 * QT - kLag + k, false);
                else fold(k - kLag, k - kLag < QT);
                if (k < QT) update(k);
                __builtin_amdgcn_sched_barrier(0);
            }
            cid = 4 * gi + g;
        }
#pragma unroll
        for (int k = 4 * QT - kLag; k < 4 * QT; ++k) fold(k, false);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) update(qt);
    }
    __syncthreads();  // every wave is done reading sA / sQB
    PCM_STAMP(3);
#ifdef PCM_STAMPS
    if (tid == 0 && blockIdx.x < 4096) g_pcm_stamps[(8192 + blockIdx.x) * 8 + 3] = __builtin_amdgcn_s_memtime();
#endif
    // raw tile for the rescans (this thread's staged targets)
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int p = tid + r * NT;
        if (p < nt) { sT[0][mslot(p)] = tv[r][0]; sT[1][mslot(p)] = tv[r][1]; sT[2][mslot(p)] = tv[r][2]; }
    }
    // the four lane groups of a wave hold the same 8 query tiles against
    // different chunks: two halving steps leave lane group g with the folded
    // partials of tiles 4 (g >> 1) + 2 (g & 1) + {0, 1}; one partial per
    // (quarter, query) to LDS
    static_assert(QT == 8, "two halving steps: 8 query tiles -> 2 per lane");
    if constexpr (kWide) {
        // the wide form: the two lane halves hold the same 4 query tiles
        // against different chunks; one step leaves lane half wh with the
        // folded partials of tiles 2 wh + {0, 1}
        static_assert(QTW == 4, "one halving step: 4 query tiles -> 2 per lane");
        int t2;  // (a copy of tid the compiler cannot see through: wc is recomputed, not carried across the loop)
        asm volatile("v_mov_b32 %0, %1" : "=v"(t2) : "v"(tid));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            mfma_fold_step<true>(best[j], sec[j], bchunk[j], best[j + 2], sec[j + 2], bchunk[j + 2]);
            const int s = half * (QW / 2) + (2 * ((t2 >> 5) & 1) + j) * 32 + (t2 & 31);
            sPB[quarter][s] = best[j];
            sPS[quarter][s] = sec[j];
            sPC[quarter][s] = bchunk[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            mfma_fold_step<true>(best[j], sec[j], bchunk[j], best[j + 4], sec[j + 4], bchunk[j + 4]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            mfma_fold_step<false>(best[j], sec[j], bchunk[j], best[j + 2], sec[j + 2], bchunk[j + 2]);
            const int s = half * (QW / 2) + (4 * (g >> 1) + 2 * (g & 1) + j) * 16 + col;
            sPB[quarter][s] = best[j];
            sPS[quarter][s] = sec[j];
            sPC[quarter][s] = bchunk[j];
        }
    }
    const int any_nonfinite = pcm_wg_or(nonfinite, sNFm, W);
    PCM_STAMP(4);

    float my_d = 0.f;
    if (!any_nonfinite) {
        // ---- one pass, one barrier: thread (s = tid mod QW, part = tid / QW)
        // merges the four quarters' partials of query s -- both parts reach
        // the same verdict and the same plan -- and, when the best chunk is
        // proven, rescans its half of that chunk exactly (tiles 2 part,
        // 2 part + 1 of the group, rows 4g..4g+3, ascending).  A wave then
        // scans the near ties among its 64 queries itself, in turn with the
        // other part's wave.
        const int s = tid & (QW - 1), part = tid / QW;
        {
            float vb[4], vs[4], vr[W];
            int vc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // every load first, then branch-free selects
                vb[q] = sPB[q][s];
                vs[q] = sPS[q][s];
                vc[q] = sPC[q][s];
            }
#pragma unroll
            for (int w = 0; w < W; ++w) vr[w] = sRmax[w];
            __builtin_amdgcn_sched_barrier(0);
            float fb = vb[0], fs = vs[0];
            int fc = vc[0];
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const bool better = (vb[q] < fb) | ((vb[q] == fb) & (vc[q] < fc));
                fs = __builtin_fminf(__builtin_fminf(fs, vs[q]), better ? fb : vb[q]);
                fb = better ? vb[q] : fb;
                fc = better ? vc[q] : fc;
            }
            float rmax2 = vr[0];
#pragma unroll
            for (int w = 1; w < W; ++w) rmax2 = __builtin_fmaxf(rmax2, vr[w]);
            // the bound E of the header with R = max |t'| for every target (eR),
            // and, as filt_forward argues it, with |t'| <= |q'| + sqrt(d_b) for
            // every target that can reach the best chunk's exact minimum d_b
            // <= fb + |q'|^2 + eR: E <= 80u (2|q'| + sqrt(db))^2
            const float kAbs = 7.888609052210118e-31f;  // 2^-100
            const float qn2 = kWide ? qn2w : __builtin_fmaf(qzc, qzc, __builtin_fmaf(qyc, qyc, qxc * qxc));
            const float sq = __builtin_amdgcn_sqrtf(qn2);
            const float rr = __builtin_amdgcn_sqrtf(rmax2) + sq;
            const float eR = kFiltU80 * (rr * rr) * 1.001f + kAbs;
            const float db = __builtin_fmaxf((fb + qn2) * 1.0001f + 2.f * eR, 0.f);
            const float rq = 2.f * sq + __builtin_amdgcn_sqrtf(db);
            const float e2 = 2.f * (kFiltU80 * __builtin_fminf(rr * rr, rq * rq) * 1.001f + kAbs);
            const bool proven = (fs - fb) > e2;  // false for NaN
            const bool live = qbase + s < nq;
            // near-tie plan: quarter q is scanned whole (bit q) when its
            // second-best chunk may lie within fb + 2E, else its best chunk
            // alone (bit 4 + q) when that one may; every other candidate
            // screens above fb + 2E, so lies above the answer.  NaN anywhere
            // selects the scan.
            const float thr = fb + e2;
            unsigned plan = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) plan |= !(vs[q] > thr) ? (1u << q) : (!(vb[q] > thr) ? (16u << q) : 0u);
            float hd = PCM_INF;
            int hk = 0x7fffffff;
            if (live) {
                if (proven) {
                    // two quads of the raw tile, 16 targets apart; a quad stays
                    // contiguous under mslot, and slots past nt (inside the last
                    // 64-target group) hold stale bytes that `take` ignores
                    // (the wide form's chunk: A tile (fc >> 1) & 1 of the group,
                    // lane half fc & 1 -- rows 8 j + 4 (fc & 1) + r, j = 2 part,
                    // 2 part + 1: two quads 8 targets apart)
                    constexpr int kQuad = kWide ? 8 : 16;
                    const int k0 = kWide ? 64 * (fc >> 2) + 32 * ((fc >> 1) & 1) + 4 * (fc & 1) + 16 * part
                                         : 64 * (fc >> 2) + 32 * part + 4 * (fc & 3);
                    pcm_f4 tx[2], ty[2], tz[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int o = mslot(k0 + kQuad * h);
                        tx[h] = *reinterpret_cast<const pcm_f4 *>(&sT[0][o]);
                        ty[h] = *reinterpret_cast<const pcm_f4 *>(&sT[1][o]);
                        tz[h] = *reinterpret_cast<const pcm_f4 *>(&sT[2][o]);
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {  // ascending: strict '<' keeps the lowest
                        const int kk = k0 + kQuad * (k >> 2) + (k & 3);
                        const float d = pcm_sqd(tx[k >> 2][k & 3] - qx, ty[k >> 2][k & 3] - qy, tz[k >> 2][k & 3] - qz);
                        const bool take = (d < hd) & (kk < nt);
                        hd = take ? d : hd;
                        hk = take ? kk : hk;
                    }
                }
            }
            PCM_STAMP(5);
            // ---- near ties, inside the wave that holds the query: waves w
            // and w + 4 hold the same 64 queries (parts 0 and 1) and see the
            // same mask; its j-th set bit falls to part j & 1, whose wave
            // scans that query's whole plan exactly and hands the result to
            // the query's own lane, while the other part keeps (+inf, none):
            // the outputs take the lexmin of the two parts, as for a proven
            // query.  The query, its plan and its quarters' best chunks come
            // from the listed lane's registers.  One step takes the four
            // quarters' single chunks (lane group q: the 16 targets of quarter
            // q's best chunk); a whole quarter is its up to four 64-target
            // groups, one target per lane each.
            unsigned long long todo = __builtin_amdgcn_ballot_w64(live && !proven);
            const int wpart = wave / QPT;  // this wave's part, wave-uniform
#ifdef PCM_STAMPS
            {  // census (each query once: the part-0 waves count) and this wave's iterations
                const bool on = live && !proven && wpart == 0;
                const int nfull = wave_sum_dpp(on ? (int)__popc(plan & 15u) : 0);
                const int nsingle = wave_sum_dpp(on ? (int)__popc((plan >> 4) & 15u) : 0);
                if (lane == 0) {
                    const unsigned cnt = (unsigned)__popcll(todo);
                    if (wpart == 0) {
                        atomicAdd(&sCensus[0], cnt);
                        atomicAdd(&sCensus[1], (unsigned)nfull);
                        atomicAdd(&sCensus[2], (unsigned)nsingle);
                    }
                    atomicMax(&sCensus[3], (cnt + 1u - (unsigned)wpart) >> 1);
                }
            }
#endif
            for (int j = 0; todo != 0; ++j) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1;
                if ((j & 1) != wpart) continue;
                // (the lane, opaque per iteration: from a loop-invariant lane
                // hipcc computes all sixteen whole-quarter slots and masks
                // ahead of the loop -- 270 instructions and SGPR spills, 0.7 us
                // in every wave that holds a near tie, most of which scan no
                // whole quarter; section 3.5c)
                int ln = lane;
                asm volatile("" : "+v"(ln));
                const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qx), l));
                const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qy), l));
                const float z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qz), l));
                const unsigned pl = (unsigned)__builtin_amdgcn_readlane((int)plan, l);
                float bd = PCM_INF;
                int bk = 0x7fffffff;
                {
                    const int p0 = __builtin_amdgcn_readlane(vc[0], l), p1 = __builtin_amdgcn_readlane(vc[1], l);
                    const int p2 = __builtin_amdgcn_readlane(vc[2], l), p3 = __builtin_amdgcn_readlane(vc[3], l);
                    const int pc = g == 0 ? p0 : g == 1 ? p1 : g == 2 ? p2 : p3;
                    const int k = kWide ? 64 * (pc >> 2) + 32 * ((pc >> 1) & 1) + 4 * (pc & 1) + 8 * (col >> 2) + (col & 3)
                                        : 64 * (pc >> 2) + 16 * (col >> 2) + 4 * (pc & 3) + (col & 3);
                    const bool on = ((pl >> (4 + g)) & 1u) && k < nt;
                    const int ks = mslot(min(k, nt - 1));
                    const float d = pcm_sqd(sT[0][ks] - x, sT[1][ks] - y, sT[2][ks] - z);
                    if (on) pcm_lexmin(bd, bk, d, k);
                }
                for (int q = 0; q < 4; ++q) {
                    if (!((pl >> q) & 1u)) continue;
                    float tx[4], ty[4], tz[4];
                    int kk[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {  // the quarter's groups, all loads in flight
                        const int k = 64 * (q + 4 * u) + ln;
                        // (the group from k: not a mask per (q, u) kept across the loop)
                        kk[u] = ((k >> 6) < ngroups && k < nt) ? k : -1;
                        const int ks = mslot(min(max(kk[u], 0), nt - 1));
                        tx[u] = sT[0][ks];
                        ty[u] = sT[1][ks];
                        tz[u] = sT[2][ks];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float d = pcm_sqd(tx[u] - x, ty[u] - y, tz[u] - z);
                        if (kk[u] >= 0) pcm_lexmin(bd, bk, d, kk[u]);
                    }
                }
                pcm_wave_lexmin(bd, bk);
                hd = lane == l ? bd : hd;
                hk = lane == l ? bk : hk;
            }
            sHD[part][s] = hd;
            sHK[part][s] = hk;
        }
        __syncthreads();
        PCM_STAMP(6);
#ifdef PCM_STAMPS
        if (tid == 0 && blockIdx.x < 4096) g_pcm_stamps[(8192 + blockIdx.x) * 8 + 6] = __builtin_amdgcn_s_memtime();
        // diagnostics: near ties (bits 0-15), whole quarters (16-31), the most
        // loop iterations of one wave (32-39), single chunks (40 up)
        if (tid == NT - 1 && blockIdx.x < kStampSlots)
            g_pcm_stamps[blockIdx.x * 8 + 0] = (unsigned long long)sCensus[0] | ((unsigned long long)sCensus[1] << 16) |
                                               ((unsigned long long)sCensus[3] << 32) |
                                               ((unsigned long long)sCensus[2] << 40);
#endif
        // ---- outputs (thread tid < QW is part 0 of query tid): the nearer of the two parts' results
        if (tid < QW && qbase + tid < nq) {
            float d = sHD[0][tid];
            int k = sHK[0][tid];
            pcm_lexmin(d, k, sHD[1][tid], sHK[1][tid]);
            my_d = d;
            out_st<kSc1>(D + qbase + tid, d);
            out_st<kSc1>(I + qbase + tid, (int32_t)k);
            // data-tagged argmin granule {call tag, idx}: one 8-byte sc1 store, its own flag
            if (Gr) __hip_atomic_store(Gr + qbase + tid, tag | (unsigned)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (kown) *kown = k;
        }
    } else {
        for (int s = tid; s < QW; s += NT) {
            const int qi = qbase + s;
            if (qi >= nq) continue;
            float d;
            int idx;
            pcm_ref_nn_scan(pcm_ld(Q + pcm_at(LQ, qi, 0)), pcm_ld(Q + pcm_at(LQ, qi, 1)),
                            pcm_ld(Q + pcm_at(LQ, qi, 2)), T, nt, d, idx, LT);
            my_d = d;
            out_st<kSc1>(D + qi, d);
            out_st<kSc1>(I + qi, (int32_t)idx);
            if (Gr) __hip_atomic_store(Gr + qi, tag | (unsigned)idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (kown) *kown = idx;
        }
    }
    return my_d;
}

// ---------------------------------------------------------------------------
// Forward kernel: direction-major workgroup numbering (as the other forward
// forms), optional loss granule (mode 3, chamfer_loss.h).
// ---------------------------------------------------------------------------
// amdgpu_waves_per_eu(4): at most 128 VGPRs, so two 512-thread workgroups fit
// a CU (left to itself hipcc spends 200+ VGPRs on the epilogue's unrolled
// loads and halves the occupancy of the scan)
template <typename TIn, int W, int QPT, int C, int TILE, int kLoss>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(4))) void chamfer_fwd_filt_kernel(
    const TIn *__restrict__ xyz1, const TIn *__restrict__ xyz2, int b, int n, int m,
    float *__restrict__ dist1, float *__restrict__ dist2, int32_t *__restrict__ idx1,
    int32_t *__restrict__ idx2, int nblk1, int nblk2, float *__restrict__ partials,
    unsigned *__restrict__ ticket, float *__restrict__ mean_out) {
    static_assert(kLoss == 0 || kLoss == 3, "filtered forward publishes granules only");
    static_assert(W <= 16, "sRed holds 16 waves");
    constexpr int QW = 64 * QPT;
    __shared__ float sRed[2][16];

    int nprod = (int)gridDim.x;
    unsigned epoch = 0;
    if constexpr (kLoss == 3) {
        nprod -= 1;
        if ((int)blockIdx.x == nprod) {  // the grid's last workgroup polls
            poll_loss(b * nblk1, nprod, b, n, m, reinterpret_cast<const unsigned long long *>(partials), ticket,
                      mean_out);
            return;
        }
        epoch = ticket[kEpochWord] + 1u;  // plain load: written by an earlier launch
    }
    PCM_STAMP(0);
    // batch-major placement (both directions of an element on one XCD); the
    // loss partial's slot stays direction-major, so the poll sums in the same order
    int batch, blk;
    bool first;
    pcm_split_bm(pcm_xcd_remap((int)blockIdx.x, nprod), nblk1, nblk2, batch, first, blk);
    const int slot = first ? batch * nblk1 + blk : b * nblk1 + batch * nblk2 + blk;
    const TIn *Q = first ? xyz1 + (size_t)batch * n * 3 : xyz2 + (size_t)batch * m * 3;
    const TIn *T = first ? xyz2 + (size_t)batch * m * 3 : xyz1 + (size_t)batch * n * 3;
    float *D = first ? dist1 + (size_t)batch * n : dist2 + (size_t)batch * m;
    int32_t *I = first ? idx1 + (size_t)batch * n : idx2 + (size_t)batch * m;
    const int nq = first ? n : m, nt = first ? m : n;
    const float my_d = filt_forward<TIn, W, QPT, C, TILE, false>(Q, T, nq, nt, blk * QW, D, I,
                                                                 lds_arena<FiltLds<W, QPT, TILE>::kBytes>());
    if constexpr (kLoss == 3) publish_partial<3>(my_d, slot, partials, ticket, sRed, epoch);
#ifdef PCM_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < kStampSlots)
        g_pcm_stamps[blockIdx.x * 8 + 7] = __builtin_amdgcn_s_memrealtime();
#endif
}

// The filtered forward on clouds of either layout (pcm_common.h PcmLay):
// lay1 / lay2 = 1 when that cloud is [b, 3, n] channel planes -- the
// generator's B x 3 x N output, which train.py:163 hands to the loss as a
// transposed view; the reference's wrapper copies it to rows first
// (dist_chamfer_3D.py:79-80), this reads it in place.  Same results as
// pcm_chamfer_forward on the rows, bit for bit (the same arithmetic on the
// same values).
// (the layouts are template arguments: a row stride known at compile time
// lets the loads of a point's three coordinates merge)
template <int W, int QPT, int C, int TILE, int LAY1, int LAY2>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(4))) void chamfer_fwd_filt_lay_kernel(
    const float *__restrict__ xyz1, const float *__restrict__ xyz2, int b, int n, int m,
    float *__restrict__ dist1, float *__restrict__ dist2, int32_t *__restrict__ idx1,
    int32_t *__restrict__ idx2, int nblk1, int nblk2) {
    constexpr int QW = 64 * QPT;
    int batch, blk;
    bool first;
    pcm_split_bm(pcm_xcd_remap((int)blockIdx.x, (int)gridDim.x), nblk1, nblk2, batch, first, blk);
    const float *X1 = xyz1 + (size_t)batch * n * 3, *X2 = xyz2 + (size_t)batch * m * 3;
    const PcmLay L1 = LAY1 ? PcmLay{1, n} : PcmLay{3, 1}, L2 = LAY2 ? PcmLay{1, m} : PcmLay{3, 1};
    if (first)
        filt_forward<float, W, QPT, C, TILE, false>(X1, X2, n, m, blk * QW, dist1 + (size_t)batch * n,
                                                   idx1 + (size_t)batch * n, lds_arena<FiltLds<W, QPT, TILE>::kBytes>(),
                                                   nullptr, 0, nullptr, nullptr, L1, L2);
    else
        filt_forward<float, W, QPT, C, TILE, false>(X2, X1, m, n, blk * QW, dist2 + (size_t)batch * m,
                                                   idx2 + (size_t)batch * m, lds_arena<FiltLds<W, QPT, TILE>::kBytes>(),
                                                   nullptr, 0, nullptr, nullptr, L2, L1);
}

// ---------------------------------------------------------------------------
// Fused loss + gradient
// ---------------------------------------------------------------------------
constexpr int kGradCap = 1024;   // points per cloud the per-element backward holds in LDS
// 4-byte argmin granules (variants 14, 15, 13): {tag (21 bits) << 11 | idx}
constexpr unsigned kG4TagBits = 21;
constexpr unsigned kG4TagMask = (1u << kG4TagBits) - 1u;
static_assert(kGradCap <= 2048, "a 4-byte granule holds an 11-bit index");
// Bound of a gradient-phase wait on the other workgroups' argmins (polls of
// about a microsecond each): past it the workgroup computes what is missing
// itself.  The loss poll (pcm_loss::kPollMaxSpins) waits longer: its
// producers finish within this bound plus their local scans.
constexpr unsigned kGradWaitSpins = 1u << 16;
constexpr int kGradSlots = 8;    // inverse-index entries per target sorted by the fast network
// entries per target kept in LDS: 9..16 sources take a wider in-thread sort
// (random clouds: about 2 targets per launch have more than 8; with 8 slots
// each cost its workgroup the ballot path, ~1 us, often on the kernel's
// critical path); more than 16 (a collapsed cloud): the ballot path
constexpr int kGradSlotsMax = 16;
// arena of the per-element backward: both clouds (AoS floats), a count per
// point, kGradSlots 16-bit source ids per point
constexpr int kGradBytes = 2 * kGradCap * 12 + 2 * kGradCap * 4 + 2 * kGradCap * kGradSlots * 2;

// write-through / L1-bypassing accesses of the bytes handed between
// workgroups (MI355X_MICROARCH.md, inter-workgroup visibility: sc1 stores,
// drained, then sc1 loads to registers by the consumer)
__device__ __forceinline__ int32_t ld_sc1(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sum of the scatter terms -h (A[src] - s) over the <= kGradSlots sources of
// one target (ids in tab, in arbitrary order) in ascending source index -- the
// reference's fp32 accumulation made deterministic.  The ids are sorted with
// Batcher's 19-comparator network in registers; the first four sources'
// coordinates are gathered together (clamped, unconditional LDS reads), the
// rare rest one by one.  (Measured and rejected: both clouds' targets of a
// round interleaved in straight-line code -- 2.6 -> 3.0 us per batch element.)
// getA(i, x, y, z): the coordinates of source i of the other cloud
template <typename GetA, typename GetH>
__device__ __forceinline__ void scatter_sum(float &ax, float &ay, float &az, float sx, float sy, float sz,
                                            GetH h, GetA getA, const uint16_t *tab, int cnt) {
    static_assert(kGradSlots == 8 && kGradSlotsMax == 16, "sorting networks for 8 and 16 ids");
    if (cnt > kGradSlots) {
        // rare: 9..16 sources.  Odd-even transposition sort of the two rows
        // (16 rounds), then the sum in ascending source order, one by one
        int f[16];
        const uint4 r0 = *reinterpret_cast<const uint4 *>(tab);
        const uint4 r1 = *reinterpret_cast<const uint4 *>(tab + 8);
        const unsigned wv[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int t = (int)((wv[u >> 1] >> (16 * (u & 1))) & 0xffffu);
            f[u] = u < cnt ? t : 0x7fffffff;
        }
#pragma unroll
        for (int rd = 0; rd < 16; ++rd)
#pragma unroll
            for (int i = rd & 1; i + 1 < 16; i += 2) {
                const int lo = min(f[i], f[i + 1]), hi = max(f[i], f[i + 1]);
                f[i] = lo;
                f[i + 1] = hi;
            }
        for (int u = 0; u < cnt; ++u) {
            float tx, ty, tz;
            getA(f[u], tx, ty, tz);
            const float hu = h(f[u]);
            ax = __fadd_rn(ax, -__fmul_rn(hu, __fsub_rn(tx, sx)));
            ay = __fadd_rn(ay, -__fmul_rn(hu, __fsub_rn(ty, sy)));
            az = __fadd_rn(az, -__fmul_rn(hu, __fsub_rn(tz, sz)));
        }
        return;
    }
    int e[8];
    // the whole 16-byte row in one ds_read_b128; slots past cnt hold stale ids
    const uint4 row = *reinterpret_cast<const uint4 *>(tab);
    const unsigned w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int t = (int)((w[u >> 1] >> (16 * (u & 1))) & 0xffffu);
        e[u] = u < cnt ? t : 0x7fffffff;
    }
    auto cas = [&](int i, int j) {
        const int lo = min(e[i], e[j]), hi = max(e[i], e[j]);
        e[i] = lo;
        e[j] = hi;
    };
    cas(0, 1); cas(2, 3); cas(4, 5); cas(6, 7); cas(0, 2); cas(1, 3); cas(4, 6); cas(5, 7); cas(1, 2);
    cas(5, 6); cas(0, 4); cas(3, 7); cas(1, 5); cas(2, 6); cas(1, 4); cas(3, 6); cas(2, 4); cas(3, 5);
    cas(3, 4);
    auto add = [&](float hu, float tx, float ty, float tz) {
        ax = __fadd_rn(ax, -__fmul_rn(hu, __fsub_rn(tx, sx)));
        ay = __fadd_rn(ay, -__fmul_rn(hu, __fsub_rn(ty, sy)));
        az = __fadd_rn(az, -__fmul_rn(hu, __fsub_rn(tz, sz)));
    };
    float gx[4], gy[4], gz[4], gh[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int su = u < cnt ? e[u] : 0;
        getA(su, gx[u], gy[u], gz[u]);
        gh[u] = h(su);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool on = u < cnt;
        const float nx = __fadd_rn(ax, -__fmul_rn(gh[u], __fsub_rn(gx[u], sx)));
        const float ny = __fadd_rn(ay, -__fmul_rn(gh[u], __fsub_rn(gy[u], sy)));
        const float nz = __fadd_rn(az, -__fmul_rn(gh[u], __fsub_rn(gz[u], sz)));
        ax = on ? nx : ax;
        ay = on ? ny : ay;
        az = on ? nz : az;
    }
    for (int u = 4; u < cnt; ++u) {
        float tx, ty, tz;
        getA(e[u], tx, ty, tz);
        add(h(e[u]), tx, ty, tz);
    }
}

// ---------------------------------------------------------------------------
// Standalone backward with per-point graddists (pcm_chamfer_backward's default
// for clouds of <= kBwdSlotsMax points): the 256-target workgroup layout of
// chamfer.hip's staged kernel -- the other cloud's argmins, points and
// graddists arrive by LDS-DMA -- but the sources are bucketed the fused step's
// way (range_grad): one LDS atomic claims a slot of the target's 16-slot row,
// and the target's thread sorts its row and sums in ascending source order
// (scatter_sum), instead of a histogram, a scan, a fill and a rank pass with a
// barrier each.  A target with more than 16 sources (a collapsed cloud) sums
// by an ordered scan of the other cloud's argmins.  Same arithmetic and order
// as the reference's kernels (chamfer3D.cu:155-195), bit-identical.
// ---------------------------------------------------------------------------
//
// Rescale mode (RS.gl != nullptr; pcm_chamfer_loss_grad_rescale): the backward
// of a one-launch step (pcm_chamfer_loss_grad_layout) whose gradient was
// computed for an expected upstream scale *RS.used.  If the real upstream
// gradient *RS.gl has the same bits, the step's gradient is already exact and
// every workgroup returns at once; otherwise this recomputes it with the
// scalar graddists fl(*RS.gl * inv) -- torch's mean backward -- in place.
// Either way *RS.next = *RS.gl (the next step's expectation).
// ---------------------------------------------------------------------------
constexpr int kBwdSlotsT = 256;      // targets per workgroup = threads
constexpr int kBwdSlotsMax = 2048;   // points of the other cloud staged in LDS

struct PcmRescale {
    const float *gl = nullptr;    // device: the upstream gradient of the loss
    const float *used = nullptr;  // device: the scale the step used (nullptr: always recompute)
    float *next = nullptr;        // device: receives *gl (nullable)
    float inv1 = 0.f, inv2 = 0.f; // fl(1 / (b n)), fl(1 / (b m))
};

// One 256-target block (task) of the slot backward; every thread of the
// workgroup takes part (the caller's loop may run several tasks in a row).
__device__ __forceinline__ void slots_task(int task, int ntasks, const float *__restrict__ xyz1,
                                           const float *__restrict__ xyz2, int n, int m,
                                           const float *__restrict__ gd1, const float *__restrict__ gd2,
                                           const int32_t *__restrict__ idx1, const int32_t *__restrict__ idx2,
                                           float *__restrict__ grad1, float *__restrict__ grad2, int nblk1, int nblk2,
                                           int lay1, int lay2, PcmGdStr GS, bool rescale, float rs1, float rs2) {
    constexpr int NT = kBwdSlotsT;
    __shared__ __attribute__((aligned(16))) float sO[3 * kBwdSlotsMax];  // other cloud, its layout
    __shared__ __attribute__((aligned(16))) float sG[kBwdSlotsMax];      // other graddist
    __shared__ __attribute__((aligned(16))) int sK[kBwdSlotsMax];        // other argmins
    __shared__ int cnt[NT];
    __shared__ __attribute__((aligned(16))) uint16_t tab[NT * kGradSlotsMax];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    int batch, blk;
    bool first;
    pcm_split_bm(pcm_xcd_remap(task, ntasks), nblk1, nblk2, batch, first, blk);
    const int ns = first ? n : m, no = first ? m : n;
    const float rs_self = first ? rs1 : rs2, rs_other = first ? rs2 : rs1;
    const float *self = first ? xyz1 + (size_t)batch * n * 3 : xyz2 + (size_t)batch * m * 3;
    const float *other = first ? xyz2 + (size_t)batch * m * 3 : xyz1 + (size_t)batch * n * 3;
    const int gbs = first ? (GS.bs1 < 0 ? n : GS.bs1) : (GS.bs2 < 0 ? m : GS.bs2);
    const int gbo = first ? (GS.bs2 < 0 ? m : GS.bs2) : (GS.bs1 < 0 ? n : GS.bs1);
    const int gps = rescale ? 0 : (first ? GS.ps1 : GS.ps2), gpo = rescale ? 0 : (first ? GS.ps2 : GS.ps1);
    const float *gds = (first ? gd1 : gd2) + (size_t)batch * gbs;  // (not read in rescale mode)
    const float *gdo = (first ? gd2 : gd1) + (size_t)batch * gbo;
    const int32_t *ids = (first ? idx1 + (size_t)batch * n : idx2 + (size_t)batch * m);
    const int32_t *ido = (first ? idx2 + (size_t)batch * m : idx1 + (size_t)batch * n);
    float *grad = first ? grad1 + (size_t)batch * n * 3 : grad2 + (size_t)batch * m * 3;
    const PcmLay LS = first ? pcm_lay(lay1, n) : pcm_lay(lay2, m);
    const PcmLay LO = first ? pcm_lay(lay2, m) : pcm_lay(lay1, n);
    const int t0 = blk * NT;
    const int T = min(NT, ns - t0);

    pcm_dma_to_lds(sK, ido, 4 * no, wave, NT / 64);
    pcm_dma_to_lds(sO, other, 12 * no, wave, NT / 64);
    // graddists of the other cloud: by LDS-DMA when contiguous, one register
    // when an expanded scalar (stride 0), else strided loads
    float hconst = 0.f;
    if (rescale)
        hconst = __fmul_rn(rs_other, 2.f);
    else if (gpo == 1)
        pcm_dma_to_lds(sG, gdo, 4 * no, wave, NT / 64);
    else if (gpo == 0)
        hconst = __fmul_rn(gdo[0], 2.f);
    else
        for (int j = tid; j < no; j += NT) sG[j] = gdo[(size_t)j * gpo];
    const int i = t0 + tid;
    const bool own = tid < T;
    float sx = 0.f, sy = 0.f, sz = 0.f, gself = 0.f;
    int kself = 0;
    if (own) {
        sx = self[pcm_at(LS, i, 0)];
        sy = self[pcm_at(LS, i, 1)];
        sz = self[pcm_at(LS, i, 2)];
        kself = ids[i];
        gself = rescale ? rs_self : gds[(size_t)i * gps];
    }
    cnt[tid] = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // every source whose argmin falls in [t0, t0 + T) claims a slot of its row
    for (int j = tid; j < no; j += NT) {
        const unsigned k = (unsigned)(sK[j] - t0);
        if (k < (unsigned)T) {
            const int slot = atomicAdd(&cnt[k], 1);
            if (slot < kGradSlotsMax) tab[k * kGradSlotsMax + slot] = (uint16_t)j;
        }
    }
    __syncthreads();
    if (!own) return;  // (no barrier follows inside the task)
    const float g = __fmul_rn(gself, 2.f);
    const float d0 = __fmul_rn(g, __fsub_rn(sx, sO[pcm_at(LO, kself, 0)]));
    const float d1 = __fmul_rn(g, __fsub_rn(sy, sO[pcm_at(LO, kself, 1)]));
    const float d2 = __fmul_rn(g, __fsub_rn(sz, sO[pcm_at(LO, kself, 2)]));
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (first) {  // cloud 1: direct term first (chamfer3D.cu:184), then the cloud-2 scatters
        ax = __fadd_rn(ax, d0);
        ay = __fadd_rn(ay, d1);
        az = __fadd_rn(az, d2);
    }
    auto getA = [&](int j, float &x, float &y, float &z) {
        x = sO[pcm_at(LO, j, 0)];
        y = sO[pcm_at(LO, j, 1)];
        z = sO[pcm_at(LO, j, 2)];
    };
    auto geth = [&](int j) { return gpo == 0 ? hconst : __fmul_rn(sG[j], 2.f); };
    const int c = cnt[tid];
    if (c <= kGradSlotsMax) {
        scatter_sum(ax, ay, az, sx, sy, sz, geth, getA, tab + tid * kGradSlotsMax, c);
    } else {
        // a collapsed cloud: the other cloud's sources of this target in ascending order
        for (int j = 0; j < no; ++j)
            if (sK[j] == i) {
                const float h = geth(j);
                ax = __fadd_rn(ax, -__fmul_rn(h, __fsub_rn(sO[pcm_at(LO, j, 0)], sx)));
                ay = __fadd_rn(ay, -__fmul_rn(h, __fsub_rn(sO[pcm_at(LO, j, 1)], sy)));
                az = __fadd_rn(az, -__fmul_rn(h, __fsub_rn(sO[pcm_at(LO, j, 2)], sz)));
            }
    }
    if (!first) {  // cloud 2: the cloud-1 scatters first (kernel 1 ran before kernel 2), then direct
        ax = __fadd_rn(ax, d0);
        ay = __fadd_rn(ay, d1);
        az = __fadd_rn(az, d2);
    }
    grad[pcm_at(LS, i, 0)] = ax;
    grad[pcm_at(LS, i, 1)] = ay;
    grad[pcm_at(LS, i, 2)] = az;
}

// Rescale mode (RS.gl): a small grid whose workgroups loop over the tasks --
// almost always it only confirms the scale and leaves, and the rare recompute
// (a loop's first step, a changed weight) can afford fewer workgroups.
constexpr int kRescaleGrid = 32;

__global__ __launch_bounds__(kBwdSlotsT) void chamfer_bwd_slots_kernel(
    const float *__restrict__ xyz1, const float *__restrict__ xyz2, int b, int n, int m,
    const float *__restrict__ gd1, const float *__restrict__ gd2, const int32_t *__restrict__ idx1,
    const int32_t *__restrict__ idx2, float *__restrict__ grad1, float *__restrict__ grad2, int nblk1, int nblk2,
    int lay1, int lay2, PcmGdStr GS, PcmRescale RS) {
    const int ntasks = b * (nblk1 + nblk2);
    if (RS.gl) {
        const float gl = *RS.gl;
        if (RS.next && blockIdx.x == 0 && threadIdx.x == 0) *RS.next = gl;
        if (RS.used && __float_as_uint(*RS.used) == __float_as_uint(gl)) return;  // the step's gradient stands
        const float rs1 = __fmul_rn(gl, RS.inv1), rs2 = __fmul_rn(gl, RS.inv2);
        for (int t = (int)blockIdx.x; t < ntasks; t += (int)gridDim.x) {
            slots_task(t, ntasks, xyz1, xyz2, n, m, gd1, gd2, idx1, idx2, grad1, grad2, nblk1, nblk2, lay1, lay2, GS,
                       true, rs1, rs2);
            __syncthreads();  // the next task reuses the LDS
        }
        return;
    }
    slots_task((int)blockIdx.x, ntasks, xyz1, xyz2, n, m, gd1, gd2, idx1, idx2, grad1, grad2, nblk1, nblk2, lay1,
               lay2, GS, false, 0.f, 0.f);
}

// Gradients of L = w1 sum(dist1) + w2 sum(dist2) for the targets
// [q0, q0 + QW) of ONE cloud -- the query range this workgroup's forward
// covered -- with both clouds in LDS (chamfer3D.cu:155-195, g = 2 w):
//   cloud 1:  grad1[j] = g1 (p_j - q_I1[j])  then  - g2 (q_k - p_j) for k in S2(j) ascending
//   cloud 2:  grad2[k] = - g1 (p_j - q_k) for j in S1(k) ascending  then  g2 (q_k - p_I2[k])
// S2(j) = {k : I2[k] = j}, S1(k) = {j : I1[j] = k}.  Every source of the
// other cloud whose argmin falls in the range claims a slot of its target's
// bucket with one LDS atomic; the target's thread orders them.  A target with
// more than kGradSlots sources (random clouds: ~1 in 30k; a collapsed cloud:
// all of them) is finished by the whole workgroup: ballots list its sources in
// ascending order, one thread sums them.  Identical bits to
// chamfer_bwd_staged_kernel fed graddist = w.
// S / A: the range's cloud and the other cloud (LDS); nq / na their sizes;
// gs / h: 2w of the range's direction (direct term) and of the other one
// (scatter terms); Iown / Ioth: the argmins (written by other workgroups: sc1).
//
// kLocalC > 0 (granule form, a resident forward): nothing is copied in.  The
// other cloud is the forward's own target tile, still in LDS as raw (x, y, z,
// 0) rows at filt_slot<kLocalC>(i) (TA), and the range's points are the
// forward's queries (SO[slot]); S and A are then the GLOBAL clouds, read only
// by the timeout path's local argmin scans.
// kG4: 4-byte granules {tag (21 bits) << 11 | idx} (tag: the u32 tag << 11)
// instead of 8-byte {tag, idx}; own_k >= 0: this thread's own argmin is
// already known (the workgroup's forward computed it), no granule read.
template <int NT, int QW, bool kGran = false, int kLocalC = 0, bool kG4 = false>
__device__ __forceinline__ bool range_grad(bool dir1, int q0, int nq, int na, const float *S, const float *A,
                                           float gs, float h, const int32_t *__restrict__ Iown,
                                           const int32_t *__restrict__ Ioth, float *__restrict__ G,
                                           unsigned char *scratch,
                                           const void *__restrict__ Gown_v = nullptr,
                                           const void *__restrict__ Goth_v = nullptr,
                                           unsigned long long tag = 0, unsigned max_spins = 0,
                                           unsigned *slow = nullptr, const pcm_f4 *TA = nullptr,
                                           const pcm_f4 *SO = nullptr, int own_k = -1,
                                           PcmLay LS = PcmLay{3, 1}, PcmLay LA = PcmLay{3, 1},
                                           PcmLay LG = PcmLay{3, 1}) {
    typedef typename std::conditional<kG4, unsigned, unsigned long long>::type gran_t;
    const gran_t *Gown = reinterpret_cast<const gran_t *>(Gown_v);
    const gran_t *Goth = reinterpret_cast<const gran_t *>(Goth_v);
    auto tag_of = [](gran_t v) -> unsigned {
        if constexpr (kG4) return (unsigned)v >> 11;
        else return (unsigned)((unsigned long long)v >> 32);
    };
    auto idx_of = [](gran_t v) -> int {
        if constexpr (kG4) return (int)((unsigned)v & 2047u);
        else return (int)(unsigned)v;
    };
    constexpr int kPerS = (kGradCap + NT - 1) / NT;  // sources per thread
    static_assert(kLocalC > 0 || 24 * kGradCap + 4 * QW + 2 * QW * kGradSlotsMax + 4 * kGradCap <= kGradBytes,
                  "both clouds, the counts, the buckets and the overflow list fit the arena");
    static_assert(kLocalC == 0 || kGran, "local clouds: granule form");
    // coordinates of point i of the other cloud, and of the range's slot t
    auto getA = [&](int i, float &x, float &y, float &z) {
        if constexpr (kLocalC > 0) {
            const pcm_f4 t4 = TA[filt_slot<kLocalC>(i)];
            x = t4.x;
            y = t4.y;
            z = t4.z;
        } else {
            x = A[pcm_at(LA, i, 0)];
            y = A[pcm_at(LA, i, 1)];
            z = A[pcm_at(LA, i, 2)];
        }
    };
    auto getS = [&](int t, float &x, float &y, float &z) {
        if constexpr (kLocalC > 0) {
            const pcm_f4 s4 = SO[t];
            x = s4.x;
            y = s4.y;
            z = s4.z;
        } else {
            x = S[pcm_at(LS, q0 + t, 0)];
            y = S[pcm_at(LS, q0 + t, 1)];
            z = S[pcm_at(LS, q0 + t, 2)];
        }
    };
    constexpr int NW = NT / 64;
    __shared__ int sOvf[QW];   // overflowed targets (range slot)
    __shared__ int sNOvf;
    __shared__ int sWcnt[kPerS][NW];
    __shared__ int sWt[2][NW];  // the sweep's per-wave "still waiting" votes, by iteration parity
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    int *cnt = reinterpret_cast<int *>(scratch);                   // [QW] sources per target
    uint16_t *tab = reinterpret_cast<uint16_t *>(cnt + QW);        // [QW][slots]
    int *lst = reinterpret_cast<int *>(tab + QW * kGradSlotsMax);  // [na] overflow source list

    const int jt = q0 + tid;  // this thread's target (tid < QW)
    int io = 0;
    int isr[kPerS];
    if constexpr (kGran) {
        // the bucket counts are zeroed before the sweep: its vote barrier
        // (every sweep takes at least one) orders them before the bucket
        // atomics, so no barrier of their own (the caller's barrier after the
        // forward has retired every use of these LDS bytes)
        if (tid < QW) cnt[tid] = 0;
        if (tid == 0) sNOvf = 0;
        // the argmins as data-tagged granules: sweep until every one this
        // thread needs carries the call's tag (bounded; the whole workgroup
        // decides together), re-reading only those not yet current
        const bool own = tid < QW && jt < nq;
        const gran_t tagv = (gran_t)tag;
        gran_t go = !own ? tagv : (own_k >= 0 ? (gran_t)(tagv | (gran_t)own_k)
                                              : __hip_atomic_load(Gown + jt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        gran_t gr[kPerS];
#pragma unroll
        for (int r = 0; r < kPerS; ++r)
            gr[r] = __hip_atomic_load(Goth + min(tid + r * NT, na - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned want = tag_of(tagv);
        for (unsigned spins = 0;; ++spins) {
            bool ready = tag_of(go) == want;
#pragma unroll
            for (int r = 0; r < kPerS; ++r) ready &= tag_of(gr[r]) == want;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (and the caller's LDS-DMA has landed)
            const int waiting = pcm_wg_or(!ready, sWt[spins & 1u], NW);
            if (!waiting && max_spins != 0u) break;
            if (spins >= max_spins) {
                // uniform (every thread saw the same vote): the workgroups
                // that owe these argmins are not running yet (not resident,
                // or slow).  Every argmin still missing is computed here by
                // the reference-exact scan over the LDS-resident clouds --
                // the value the forward publishes -- so a timeout costs time,
                // never correctness.  max_spins == 0 (tests) recomputes all.
                const bool all = max_spins == 0u;
                if (own && (all || tag_of(go) != want)) {
                    float d, x, y, z;
                    int k;
                    getS(tid, x, y, z);
                    pcm_ref_nn_scan(x, y, z, A, na, d, k, LA);
                    go = tagv | (gran_t)k;
                }
#pragma unroll
                for (int r = 0; r < kPerS; ++r) {
                    const int i = min(tid + r * NT, na - 1);
                    if (all || tag_of(gr[r]) != want) {
                        float d, x, y, z;
                        int k;
                        getA(i, x, y, z);
                        pcm_ref_nn_scan(x, y, z, S, nq, d, k, LS);
                        gr[r] = tagv | (gran_t)k;
                    }
                }
                if (tid == 0) atomicAdd(slow, 1u);  // diagnostics (pcm_tune_chamfer_slow_paths)
                break;
            }
            __builtin_amdgcn_s_sleep(1);
            if (own && tag_of(go) != want)
                go = __hip_atomic_load(Gown + jt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int r = 0; r < kPerS; ++r)
                if (tag_of(gr[r]) != want)
                    gr[r] = __hip_atomic_load(Goth + min(tid + r * NT, na - 1), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
        }
        io = idx_of(go);
#pragma unroll
        for (int r = 0; r < kPerS; ++r) isr[r] = idx_of(gr[r]);
    } else {
        io = (tid < QW && jt < nq) ? ld_sc1(Iown + jt) : 0;
#pragma unroll
        for (int r = 0; r < kPerS; ++r) isr[r] = ld_sc1(Ioth + min(tid + r * NT, na - 1));
    }
    if constexpr (!kGran) {
        if (tid < QW) cnt[tid] = 0;
        if (tid == 0) sNOvf = 0;
        __syncthreads();
    }
    PCM_STAMP2(3);
#pragma unroll
    for (int r = 0; r < kPerS; ++r) {
        const int i = tid + r * NT;
        const int t = isr[r] - q0;
        if (i < na && (unsigned)t < (unsigned)QW) {
            const int slot = atomicAdd(&cnt[t], 1);
            if (slot < kGradSlotsMax) tab[t * kGradSlotsMax + slot] = (uint16_t)i;
        }
    }
    __syncthreads();
    PCM_STAMP2(4);
    if (tid < QW && jt < nq) {
        const int c = cnt[tid];
        if (c <= kGradSlotsMax) {
            float sx, sy, sz, ox, oy, oz;
            getS(tid, sx, sy, sz);
            getA(io, ox, oy, oz);
            const float dx = __fmul_rn(gs, __fsub_rn(sx, ox));
            const float dy = __fmul_rn(gs, __fsub_rn(sy, oy));
            const float dz = __fmul_rn(gs, __fsub_rn(sz, oz));
            float ax = 0.f, ay = 0.f, az = 0.f;
            if (dir1) {  // cloud 1: direct term first (chamfer3D.cu:184), then the cloud-2 scatters
                ax = __fadd_rn(ax, dx);
                ay = __fadd_rn(ay, dy);
                az = __fadd_rn(az, dz);
            }
            scatter_sum(ax, ay, az, sx, sy, sz, [h](int) { return h; }, getA, tab + tid * kGradSlotsMax, c);
            if (!dir1) {  // cloud 2: cloud-1 scatters first (kernel 1 ran before kernel 2), then direct
                ax = __fadd_rn(ax, dx);
                ay = __fadd_rn(ay, dy);
                az = __fadd_rn(az, dz);
            }
            G[pcm_at(LG, jt, 0)] = ax;
            G[pcm_at(LG, jt, 1)] = ay;
            G[pcm_at(LG, jt, 2)] = az;
        } else {
            sOvf[atomicAdd(&sNOvf, 1)] = tid;
        }
    }
    __syncthreads();

    // ---- overflowed buckets: ascending source list by ballots, one summing thread
    const int nov = sNOvf;
    for (int e = 0; e < nov; ++e) {
        const int t = sOvf[e];
        const int j = q0 + t;
        unsigned long long bal[kPerS];
#pragma unroll
        for (int r = 0; r < kPerS; ++r) {
            const int i = tid + r * NT;
            bal[r] = __ballot(i < na && isr[r] == j);
            if (lane == 0) sWcnt[r][wave] = __popcll(bal[r]);
        }
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int r = 0; r < kPerS; ++r) {
            int base = total;
            for (int w = 0; w < NW; ++w) {
                base += (w < wave) ? sWcnt[r][w] : 0;
                total += sWcnt[r][w];
            }
            if ((bal[r] >> lane) & 1ull) lst[base + __popcll(bal[r] & ((1ull << lane) - 1ull))] = tid + r * NT;
        }
        __syncthreads();
        if (tid == t) {  // the target's own thread holds its argmin
            float sx, sy, sz, ox, oy, oz;
            getS(t, sx, sy, sz);
            getA(io, ox, oy, oz);
            const float dx = __fmul_rn(gs, __fsub_rn(sx, ox));
            const float dy = __fmul_rn(gs, __fsub_rn(sy, oy));
            const float dz = __fmul_rn(gs, __fsub_rn(sz, oz));
            float ax = 0.f, ay = 0.f, az = 0.f;
            if (dir1) {
                ax = __fadd_rn(ax, dx);
                ay = __fadd_rn(ay, dy);
                az = __fadd_rn(az, dz);
            }
            for (int q = 0; q < total; ++q) {
                float tx, ty, tz;
                getA(lst[q], tx, ty, tz);
                ax = __fadd_rn(ax, -__fmul_rn(h, __fsub_rn(tx, sx)));
                ay = __fadd_rn(ay, -__fmul_rn(h, __fsub_rn(ty, sy)));
                az = __fadd_rn(az, -__fmul_rn(h, __fsub_rn(tz, sz)));
            }
            if (!dir1) {
                ax = __fadd_rn(ax, dx);
                ay = __fadd_rn(ay, dy);
                az = __fadd_rn(az, dz);
            }
            G[pcm_at(LG, j, 0)] = ax;
            G[pcm_at(LG, j, 1)] = ay;
            G[pcm_at(LG, j, 2)] = az;
        }
        __syncthreads();
    }
    return true;
}

// Workspace of the fused kernel (after pcm_chamfer_forward_loss's bytes, so one
// zero-filled buffer serves both): the loss epoch word and the sticky error
// word (kGradErrWord) on the first line, an arrival and a departure counter per
// batch element (both left zeroed), a partial sum per workgroup, and two 8-byte
// {epoch, sum} granules per batch element (sum of dist1, sum of dist2).
struct GradWs {
    unsigned *epoch, *bcount, *bdepart;
    float *wpart;
    unsigned long long *gran;
    unsigned long long *wg;  // granule hand-off: per-workgroup {tag, loss partial}
    unsigned long long *ig;  // granule hand-off: per-point {tag, argmin}, cloud 1 [b n] then cloud 2 [b m]
};
constexpr int kGradErrWord = 4;   // word of the first line: non-zero after the loss poll timed out (sticky)
constexpr int kGradSlowWord = 5;  // diagnostics: gradient-phase waits that timed out and computed locally
// Words 6 and 7 of the first line: the shape (n, m, granule format) and the
// batch count the argmin granules were last written under, set by the loss
// poller at the end of every granule-form call (0, 0 = a fresh zero-filled
// workspace).  A granule only tells its call by its tag, and a tag comes back
// after 2^32 calls (8-byte granules) or 2^21 (4-byte, variant 13): a position
// that a call of another shape left alone for exactly that many calls would
// pass for current.  So a call whose workspace was last used by another shape
// or granule format trusts no granule: its gradient phase computes every
// argmin it needs itself (the timeout path: exact, slow, once).
constexpr int kGradShapeWord = 6;
static_assert(kGradCap <= 4096, "grad_shape_word packs n - 1 and m - 1 into 12 bits each");
__host__ __device__ __forceinline__ unsigned grad_shape_word(int n, int m, unsigned fmt) {
    return (fmt << 24) | ((unsigned)(n - 1) << 12) | (unsigned)(m - 1);  // n, m <= 1024; fmt 1 or 2: never 0
}
__device__ __forceinline__ bool grad_ws_trusted(const unsigned *hdr, int b, int n, int m, unsigned fmt) {
    const unsigned sw = hdr[kGradShapeWord], sb = hdr[kGradShapeWord + 1];
    return (sw == 0u && sb == 0u) || (sw == grad_shape_word(n, m, fmt) && sb == (unsigned)b);
}
// each batch element's arrival and departure counters on 128-byte lines of
// their own: with all of them in one line, the 8 adds and the polls per
// element queue behind every other element's at the memory side
constexpr int kCtrStride = 32;  // unsigned words
inline size_t grad_ws_bytes(int b, long long blocks, long long pts) {
    const size_t c = (size_t)b * 128, p = ((size_t)blocks * 4 + 127) / 128 * 128;
    const size_t g = ((size_t)b * 16 + 127) / 128 * 128, wg = ((size_t)blocks * 8 + 127) / 128 * 128;
    return 128 + 2 * c + p + g + wg + (size_t)pts * 8;
}
inline GradWs grad_ws(void *base, int b, long long blocks) {
    char *p = (char *)base;
    const size_t c = (size_t)b * 128;
    GradWs w;
    w.epoch = (unsigned *)p;
    w.bcount = (unsigned *)(p + 128);
    w.bdepart = (unsigned *)(p + 128 + c);
    w.wpart = (float *)(p + 128 + 2 * c);
    w.gran = (unsigned long long *)((char *)w.wpart + ((size_t)blocks * 4 + 127) / 128 * 128);
    w.wg = (unsigned long long *)((char *)w.gran + ((size_t)b * 16 + 127) / 128 * 128);
    w.ig = (unsigned long long *)((char *)w.wg + ((size_t)blocks * 8 + 127) / 128 * 128);
    return w;
}

// the grid's last workgroup: sweep the 2b granules until all carry this
// call's epoch (bounded: NaN means on timeout), fixed-order sums, advance the
// epoch (chamfer_loss.h poll_loss, with the granules per batch element)
[[maybe_unused]] __device__ __forceinline__ void poll_grad_loss(int b, int n, int m, const GradWs &ws, float *__restrict__ mean_out,
                                               unsigned max_spins) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const unsigned epoch = ws.epoch[0] + 1u;
    float s1 = 0.f, s2 = 0.f;
    bool ok = true;
    for (int base = 0; base < 2 * b && ok; base += 64) {
        const int i = base + lane;
        unsigned long long x = (unsigned long long)epoch << 32;
        for (unsigned spins = 0;; ++spins) {
            if (i < 2 * b) x = __hip_atomic_load(ws.gran + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__all((unsigned)(x >> 32) == epoch)) break;
            if (spins >= max_spins) { ok = false; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        const float v = __uint_as_float((unsigned)x);
        if (i < 2 * b) {
            if (i & 1) s2 += v;
            else s1 += v;
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    // a timed-out sweep sets the sticky error word: from then on every call on
    // this workspace reports NaN means until the caller re-zeroes it
    // (pcm_chamfer_workspace_status tells)
    if (lane == 0) {
        if (!ok) __hip_atomic_store(ws.epoch + kGradErrWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = ok && ws.epoch[kGradErrWord] == 0u;
        const float m1 = ok ? s1 / ((float)b * (float)n) : __builtin_nanf("");
        const float m2 = ok ? s2 / ((float)b * (float)m) : __builtin_nanf("");
        mean_out[0] = m1;
        mean_out[1] = m2;
        mean_out[2] = m1 + m2;
        ws.epoch[0] = epoch;
    }
}

// granule hand-off: the grid's last workgroup sweeps the b * per per-workgroup
// {tag, partial} granules (bounded), sums them in a fixed order (lanes over
// granules, direction by the workgroup's slot, then one wave sum each) and
// advances the epoch
__device__ __forceinline__ void poll_grad_loss_wg(int b, int n, int m, int per, int nblk1, const GradWs &ws,
                                                  float *__restrict__ mean_out, unsigned max_spins,
                                                  unsigned shape_word) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const unsigned epoch = ws.epoch[0] + 1u;
    const int total = b * per;
    float s1 = 0.f, s2 = 0.f;
    bool ok = true;
    // kPollPer granules per lane in flight at once (one round trip per sweep,
    // not one per 64 granules: the last producer's partial is then summed one
    // load latency after it lands), summed per lane in ascending i -- the
    // order of a 64-wide sweep, so the means keep their bits
    constexpr int kPollPer = 8;
    for (int base = 0; base < total && ok; base += 64 * kPollPer) {
        unsigned long long x[kPollPer];
#pragma unroll
        for (int c = 0; c < kPollPer; ++c)  // past the end: ready; else not yet read
            x[c] = (unsigned long long)(base + 64 * c + lane < total ? epoch - 1u : epoch) << 32;
        for (unsigned spins = 0;; ++spins) {
            bool ready = true;
#pragma unroll
            for (int c = 0; c < kPollPer; ++c) {
                const int i = base + 64 * c + lane;
                if (i < total && (unsigned)(x[c] >> 32) != epoch)
                    x[c] = __hip_atomic_load(ws.wg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int c = 0; c < kPollPer; ++c) ready &= (unsigned)(x[c] >> 32) == epoch;
            if (__all(ready)) break;
            if (spins >= max_spins) { ok = false; break; }
            __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int c = 0; c < kPollPer; ++c) {
            const int i = base + 64 * c + lane;
            const float v = __uint_as_float((unsigned)x[c]);
            if (i < total) {
                if (i % per < nblk1) s1 += v;
                else s2 += v;
            }
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        if (!ok) __hip_atomic_store(ws.epoch + kGradErrWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = ok && ws.epoch[kGradErrWord] == 0u;
        const float m1 = ok ? s1 / ((float)b * (float)n) : __builtin_nanf("");
        const float m2 = ok ? s2 / ((float)b * (float)m) : __builtin_nanf("");
        mean_out[0] = m1;
        mean_out[1] = m2;
        mean_out[2] = m1 + m2;
        ws.epoch[kGradShapeWord] = shape_word;  // every workgroup read the old words before its partial
        ws.epoch[kGradShapeWord + 1] = (unsigned)b;
        ws.epoch[0] = epoch;
    }
}

#ifdef PCM_TUNE
#include "chamfer_lgrid.h"  // fused variant 13 (rejected, tuning build only)
#endif

// LAY1 / LAY2 (the default variant's layout instances): cloud 1 / 2 given as
// channel planes [b, 3, n] (pcm_common.h PcmLay) -- train.py:163's
// fake.transpose(2, 1) read in place -- and its gradient written in the same
// layout.  gscale (nullable, device): the upstream gradient the step is
// expected to receive; the gradients are then those of
// gscale * (w1 sum(dist1) + w2 sum(dist2)) with graddist = fl(gscale * w) as
// torch's mean backward forms it, and mean_out[3] records the scale used
// (pcm_chamfer_loss_grad_rescale checks it against the real one).
template <int W, int QPT, int C, int TILE, bool kMfma = false, bool kGran = false, bool kEarly = false,
          bool kLocal = false, bool kSplit = false, bool kG4 = false, bool kG4x = false, int LAY1 = 0, int LAY2 = 0,
          bool kLayOne = false, bool kOwnK = false, bool kWide = false>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(4))) void chamfer_loss_grad_kernel(
    const float *__restrict__ xyz1, const float *__restrict__ xyz2, int b, int n, int m, float w1, float w2,
    float *__restrict__ dist1, float *__restrict__ dist2, int32_t *__restrict__ idx1, int32_t *__restrict__ idx2,
    float *__restrict__ mean_out, float *__restrict__ grad1, float *__restrict__ grad2, int nblk1, int nblk2,
    GradWs ws, unsigned max_spins, unsigned poll_spins, const float *__restrict__ gscale) {
    static_assert((LAY1 == 0 && LAY2 == 0) || kGran,
                  "channel planes: the granule forms (the LDS copies keep each cloud's layout)");
    static_assert(!kMfma || !(kEarly || kLocal || kSplit || kG4 || kG4x),
                  "the MFMA forward: counter or 8-byte granule hand-off, both clouds copied in for the gradients");
    constexpr int QW = 64 * QPT;
    constexpr int NT = 64 * W;
    static_assert(!kMfma || (W == 8 && QPT == 4 && TILE == kMfmaTile), "the MFMA forward's fixed geometry");
    static_assert(!kWide || kMfma, "the wide screen loop: a form of the MFMA forward");
    constexpr int kFwd = kMfma ? MfmaLds::kBytes : FiltLds<W, QPT, TILE>::kBytes;
    static_assert(!kMfma || kFwd <= kGradBytes,
                  "two workgroups' LDS per CU: the polling workgroup runs beside the forward workgroups from the start");
    // kEarly: the gradient phase's clouds get an LDS region of their own, so
    // their copy is issued before the scan instead of after the forward
    // kLocal: the gradient phase reads the forward's own LDS data (its
    // target tile and its queries) instead of copying both clouds in
    constexpr int kArena = (kEarly || kLocal) ? kFwd : (kFwd > kGradBytes ? kFwd : kGradBytes);
    static_assert(!kEarly || kGran, "early cloud copy: granule hand-off form");
    static_assert(!kLocal || (kGran && !kEarly && !kMfma), "local gradient data: the granule form's forward");
    constexpr int kTileBytes = 16 * TILE;  // the forward's raw (x, y, z, 0) target rows (resident clouds)
    static_assert(!kLocal || kTileBytes + 4 * QW + 2 * QW * kGradSlotsMax + 4 * kGradCap <= kFwd,
                  "the raw tile, the counts, the buckets and the overflow list fit the forward's arena");
    static_assert(QW <= NT, "one target per thread in the gradient phase");
    __shared__ float sRed[16];
    __shared__ int sFlag, sLate;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    unsigned char *arena = lds_arena<kArena>();
    unsigned char *garena = kEarly ? lds_arena<kGradBytes, 1>() : arena;  // gradient phase
    const int nprod = (int)gridDim.x - 1;
    float gsc = 1.f;
    if (gscale) {  // graddist = fl(upstream * w), torch's mean backward (a scalar load, hidden by the forward)
        gsc = *gscale;
        w1 = __fmul_rn(gsc, w1);
        w2 = __fmul_rn(gsc, w2);
    }
    if constexpr (kWide) {
        // uniform: scalar registers carry them across the forward (the wide loop has no vector one to spare)
        w1 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(w1)));
        w2 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(w2)));
    }
    if ((int)blockIdx.x == nprod) {
        PCM_STAMP2(5);
        if constexpr (kGran)
            poll_grad_loss_wg(b, n, m, nblk1 + nblk2, nblk1, ws, mean_out, poll_spins,
                              grad_shape_word(n, m, kG4 ? 2u : 1u));
        else poll_grad_loss(b, n, m, ws, mean_out, poll_spins);
        if (gscale && threadIdx.x == 0) mean_out[3] = gsc;
        PCM_STAMP2(6);
        return;
    }
    PCM_STAMP2(0);

    // batch-major numbering: one batch element's workgroups share an XCD
    const int per = nblk1 + nblk2;
    const int bid = pcm_xcd_remap((int)blockIdx.x, nprod);
    const int batch = bid / per;
    const int r = bid - batch * per;
    const bool first = r < nblk1;
    const int q0 = (first ? r : r - nblk1) * QW;
    const float *X1 = xyz1 + (size_t)batch * n * 3;
    const float *X2 = xyz2 + (size_t)batch * m * 3;
    const PcmLay L1 = LAY1 ? PcmLay{1, n} : PcmLay{3, 1}, L2 = LAY2 ? PcmLay{1, m} : PcmLay{3, 1};
    if constexpr (kGran) {
        // ---- granule hand-off (no counters): the forward publishes every
        // argmin as a {tag, idx} granule and the workgroup's partial as a
        // {tag, sum} granule; the gradient phase sweeps the granules it needs
        const unsigned long long tag = (unsigned long long)(ws.epoch[0] + 1u) << 32;
        if (!grad_ws_trusted(ws.epoch, b, n, m, kG4 ? 2u : 1u)) max_spins = 0u;  // granules of another shape: recompute
        // kG4: 4-byte argmin granules {tag (21 bits) << 11 | idx}, cloud 1 then
        // cloud 2 (chamfer_lgrid.h's layout); the range's own argmins come
        // from this workgroup's forward (no granule read)
        const unsigned tag4 = ((ws.epoch[0] + 1u) & kG4TagMask) << 11;
        unsigned *H1 = reinterpret_cast<unsigned *>(ws.ig) + (size_t)batch * n;
        unsigned *H2 = reinterpret_cast<unsigned *>(ws.ig) + (size_t)b * n + (size_t)batch * m;
        int myk = -1;
        unsigned long long *G1 = ws.ig + (size_t)batch * n, *G2 = ws.ig + (size_t)b * n + (size_t)batch * m;
        const PreDma pre{garena, X1, 12 * n, garena + 12 * kGradCap, X2, 12 * m};
        __shared__ pcm_f4 sQown[kLocal ? QW : 1];  // kLocal: the range's points (the forward's queries)
        // 16-byte granule stores when every row start is 16-byte aligned
        const bool g4x = kG4x && ((n | m) & 3) == 0;
        float my_d;
        if constexpr (kMfma) {
            // one inlined forward: the layouts reach its prologue loads only
            my_d = filt_forward_mfma<false, kWide>(
                first ? X1 : X2, first ? X2 : X1, first ? n : m, first ? m : n, q0,
                first ? dist1 + (size_t)batch * n : dist2 + (size_t)batch * m,
                first ? idx1 + (size_t)batch * n : idx2 + (size_t)batch * m, arena, first ? G1 : G2, tag,
                first ? L1 : L2, first ? L2 : L1, kOwnK ? &myk : nullptr);
        } else if constexpr (LAY1 == LAY2) {
            const PcmLay LQ = LAY1 ? PcmLay{1, first ? n : m} : PcmLay{3, 1};
            my_d = filt_forward<float, W, QPT, C, TILE, false, kSplit>(
                first ? X1 : X2, first ? X2 : X1, first ? n : m, first ? m : n, q0,
                first ? dist1 + (size_t)batch * n : dist2 + (size_t)batch * m,
                first ? idx1 + (size_t)batch * n : idx2 + (size_t)batch * m, arena, kG4 ? nullptr : (first ? G1 : G2),
                tag, kEarly ? &pre : nullptr, kLocal ? sQown : nullptr, LQ,
                LAY1 ? PcmLay{1, first ? m : n} : PcmLay{3, 1}, kG4 ? (first ? H1 : H2) : nullptr, tag4,
                (kG4 || kOwnK) ? &myk : nullptr, g4x);
        } else if (kLayOne) {  // mixed layouts, one inlined forward with the strides in registers (tuning A/B)
            my_d = filt_forward<float, W, QPT, C, TILE, false, kSplit>(
                first ? X1 : X2, first ? X2 : X1, first ? n : m, first ? m : n, q0,
                first ? dist1 + (size_t)batch * n : dist2 + (size_t)batch * m,
                first ? idx1 + (size_t)batch * n : idx2 + (size_t)batch * m, arena, kG4 ? nullptr : (first ? G1 : G2),
                tag, kEarly ? &pre : nullptr, kLocal ? sQown : nullptr, first ? L1 : L2, first ? L2 : L1,
                kG4 ? (first ? H1 : H2) : nullptr, tag4, (kG4 || kOwnK) ? &myk : nullptr, g4x);
        } else if (first) {  // mixed layouts: each direction's strides known at compile time
            my_d = filt_forward<float, W, QPT, C, TILE, false, kSplit>(
                X1, X2, n, m, q0, dist1 + (size_t)batch * n, idx1 + (size_t)batch * n, arena, kG4 ? nullptr : G1, tag,
                kEarly ? &pre : nullptr, kLocal ? sQown : nullptr, L1, L2, kG4 ? H1 : nullptr, tag4,
                (kG4 || kOwnK) ? &myk : nullptr, g4x);
        } else {
            my_d = filt_forward<float, W, QPT, C, TILE, false, kSplit>(
                X2, X1, m, n, q0, dist2 + (size_t)batch * m, idx2 + (size_t)batch * m, arena, kG4 ? nullptr : G2, tag,
                kEarly ? &pre : nullptr, kLocal ? sQown : nullptr, L2, L1, kG4 ? H2 : nullptr, tag4,
                (kG4 || kOwnK) ? &myk : nullptr, g4x);
        }
        PCM_STAMP2(1);
        const float s = wave_sum(my_d);
        if (lane == 0) sRed[wave] = s;
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
            for (int w = 0; w < W; ++w) t += sRed[w];
            __hip_atomic_store(ws.wg + bid, tag | __float_as_uint(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // the batch element's clouds for the gradient phase (the arena is free);
        // they land during the sweep (kEarly: issued before the scan)
        if constexpr (!kEarly && !kLocal) {
            pcm_dma_to_lds(arena, X1, 12 * n, wave, W);
            pcm_dma_to_lds(arena + 12 * kGradCap, X2, 12 * m, wave, W);
        }
        PCM_STAMP2(2);
        float *G = first ? grad1 + (size_t)batch * n * 3 : grad2 + (size_t)batch * m * 3;
        const float g1 = __fmul_rn(w1, 2.f), g2 = __fmul_rn(w2, 2.f);
        bool ok;
        if constexpr (kLocal) {
            // clouds as the timeout path's global fallback; the other cloud's
            // rows and the range's points from the forward's LDS
            const pcm_f4 *TA = reinterpret_cast<const pcm_f4 *>(arena);
            if constexpr (kG4)
                ok = first ? range_grad<NT, QW, true, C, true>(true, q0, n, m, X1, X2, g1, g2, nullptr, nullptr, G,
                                                               arena + kTileBytes, H1, H2, tag4, max_spins,
                                                               ws.epoch + kGradSlowWord, TA, sQown, myk, L1, L2, L1)
                           : range_grad<NT, QW, true, C, true>(false, q0, m, n, X2, X1, g2, g1, nullptr, nullptr, G,
                                                               arena + kTileBytes, H2, H1, tag4, max_spins,
                                                               ws.epoch + kGradSlowWord, TA, sQown, myk, L2, L1, L2);
            else
                ok = first ? range_grad<NT, QW, true, C>(true, q0, n, m, X1, X2, g1, g2, nullptr, nullptr, G,
                                                         arena + kTileBytes, G1, G2, tag, max_spins,
                                                         ws.epoch + kGradSlowWord, TA, sQown)
                           : range_grad<NT, QW, true, C>(false, q0, m, n, X2, X1, g2, g1, nullptr, nullptr, G,
                                                         arena + kTileBytes, G2, G1, tag, max_spins,
                                                         ws.epoch + kGradSlowWord, TA, sQown);
        } else {
            const float *P1 = reinterpret_cast<const float *>(garena);
            const float *P2 = P1 + 3 * kGradCap;
            // (the clouds' LDS copies keep their own layouts: an element's
            // channel planes are one contiguous 3n-float block, as rows are)
            if constexpr (kG4)  // 4-byte granules; the range's own argmins from its forward
                ok = first ? range_grad<NT, QW, true, 0, true>(true, q0, n, m, P1, P2, g1, g2, nullptr, nullptr, G,
                                                               garena + 24 * kGradCap, H1, H2, tag4, max_spins,
                                                               ws.epoch + kGradSlowWord, nullptr, nullptr, myk, L1,
                                                               L2, L1)
                           : range_grad<NT, QW, true, 0, true>(false, q0, m, n, P2, P1, g2, g1, nullptr, nullptr, G,
                                                               garena + 24 * kGradCap, H2, H1, tag4, max_spins,
                                                               ws.epoch + kGradSlowWord, nullptr, nullptr, myk, L2,
                                                               L1, L2);
            else
            ok = first ? range_grad<NT, QW, true>(true, q0, n, m, P1, P2, g1, g2, nullptr, nullptr, G,
                                                  garena + 24 * kGradCap, G1, G2, tag, max_spins,
                                                  ws.epoch + kGradSlowWord, nullptr, nullptr, kOwnK ? myk : -1, L1, L2, L1)
                       : range_grad<NT, QW, true>(false, q0, m, n, P2, P1, g2, g1, nullptr, nullptr, G,
                                                  garena + 24 * kGradCap, G2, G1, tag, max_spins,
                                                  ws.epoch + kGradSlowWord, nullptr, nullptr, kOwnK ? myk : -1, L2, L1, L2);
        }
        if (!ok) {  // a workgroup of this element never published: sticky error, NaN gradients
            if (tid == 0) __hip_atomic_store(ws.epoch + kGradErrWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int nq = first ? n : m;
            const PcmLay LG = first ? L1 : L2;
            for (int t = tid; t < 3 * QW; t += NT)
                if (q0 + t / 3 < nq) G[pcm_at(LG, q0 + t / 3, t % 3)] = __builtin_nanf("");
        }
        PCM_STAMP2(7);
        return;
    }
    float my_d;
    if constexpr (kMfma)
        my_d = filt_forward_mfma<true, kWide>(first ? X1 : X2, first ? X2 : X1, first ? n : m, first ? m : n, q0,
                                              first ? dist1 + (size_t)batch * n : dist2 + (size_t)batch * m,
                                              first ? idx1 + (size_t)batch * n : idx2 + (size_t)batch * m, arena);
    else
        my_d = filt_forward<float, W, QPT, C, TILE, true>(
            first ? X1 : X2, first ? X2 : X1, first ? n : m, first ? m : n, q0,
            first ? dist1 + (size_t)batch * n : dist2 + (size_t)batch * m,
            first ? idx1 + (size_t)batch * n : idx2 + (size_t)batch * m, arena);
    PCM_STAMP2(1);

    // ---- workgroup partial (fixed order), write-through; drain; arrive
    const float s = wave_sum(my_d);
    if (lane == 0) sRed[wave] = s;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < W; ++w) t += sRed[w];
        __hip_atomic_store(ws.wpart + bid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // every storing wave drains its sc1 stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- arrive, then wait (bounded) until every workgroup of this batch
    // element has arrived: all argmins are then published.  The grid (b *
    // per + 1 workgroups of 64 W threads) is sized to be co-resident; a wait
    // that times out sets the sticky error word and yields NaN gradients.
    // The batch element's clouds for the gradient phase (L2-hot; the forward
    // is done with the arena) are fetched into LDS during the wait: issued
    // after the arrival (wave 0: after its add returned), so no arrival
    // waits for them.
    unsigned old_arrivals = 0;
    if (tid == 0) {
        old_arrivals = __hip_atomic_fetch_add(ws.bcount + (size_t)batch * kCtrStride, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    }
    pcm_dma_to_lds(arena, X1, 12 * n, wave, W);
    pcm_dma_to_lds(arena + 12 * kGradCap, X2, 12 * m, wave, W);
    if (tid == 0) {
        unsigned *ctr = ws.bcount + (size_t)batch * kCtrStride;
        unsigned *dep_ctr = ws.bdepart + (size_t)batch * kCtrStride;
        const unsigned old = old_arrivals;
        sFlag = (old == (unsigned)per - 1);
        int late = 0;
        if (old != (unsigned)per - 1) {
            for (unsigned spins = 0;; ++spins) {
                if (ld_sc1((const int32_t *)ctr) == per) break;
                if (spins >= poll_spins) { late = 1; break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        sLate = late;
        if (late) __hip_atomic_store(ws.epoch + kGradErrWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the last to leave the wait re-arms both counters for the next call
        const unsigned dep = __hip_atomic_fetch_add(dep_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dep == (unsigned)per - 1) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(dep_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the LDS-DMA has landed
    __syncthreads();
    PCM_STAMP2(2);

    // ---- the batch element's last arriver also publishes its loss sums
    // (wave 0; the granule is the flag, nothing waits on it here)
    if (sFlag && wave == 0) {
        float v1 = 0.f, v2 = 0.f;
        for (int i = lane; i < per; i += 64) {
            const float v = ld_sc1(ws.wpart + (size_t)batch * per + i);
            if (i < nblk1) v1 += v;
            else v2 += v;
        }
        v1 = wave_sum(v1);
        v2 = wave_sum(v2);
        if (lane < 2) {
            const unsigned long long tag = (unsigned long long)(ws.epoch[0] + 1u) << 32;
            __hip_atomic_store(ws.gran + 2 * batch + lane, tag | __float_as_uint(lane ? v2 : v1), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    float *G = first ? grad1 + (size_t)batch * n * 3 : grad2 + (size_t)batch * m * 3;
    if (sLate) {  // the argmins of the other direction may be missing
        const int nq = first ? n : m;
        for (int t = tid; t < 3 * QW; t += NT)
            if (q0 * 3 + t < 3 * nq) G[3 * q0 + t] = __builtin_nanf("");
        return;
    }
    // ---- gradients of this workgroup's query range
    const float *P1 = reinterpret_cast<const float *>(arena);
    const float *P2 = P1 + 3 * kGradCap;
    const float g1 = __fmul_rn(w1, 2.f), g2 = __fmul_rn(w2, 2.f);
    if (first)
        range_grad<NT, QW>(true, q0, n, m, P1, P2, g1, g2, idx1 + (size_t)batch * n, idx2 + (size_t)batch * m, G,
                           arena + 24 * kGradCap);
    else
        range_grad<NT, QW>(false, q0, m, n, P2, P1, g2, g1, idx2 + (size_t)batch * m, idx1 + (size_t)batch * n, G,
                           arena + 24 * kGradCap);
    PCM_STAMP2(7);
}

}  // namespace

// the slot-bucket backward (above); the caller (chamfer.hip launch_bwd) has
// checked the shapes and pointers, n, m > 0
bool pcm_bwd_slots_fits(int n, int m) { return n <= kBwdSlotsMax && m <= kBwdSlotsMax; }
int pcm_launch_bwd_slots(const float *xyz1, const float *xyz2, int b, int n, int m, const float *gd1, const float *gd2,
                         const int32_t *idx1, const int32_t *idx2, float *grad1, float *grad2, int lay1, int lay2,
                         PcmGdStr GS, hipStream_t stream) {
    const int nblk1 = (n + kBwdSlotsT - 1) / kBwdSlotsT, nblk2 = (m + kBwdSlotsT - 1) / kBwdSlotsT;
    const long long blocks = (long long)b * (nblk1 + nblk2);
    if (blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(chamfer_bwd_slots_kernel, dim3((unsigned)blocks), dim3(kBwdSlotsT), 0, stream, xyz1, xyz2, b,
                       n, m, gd1, gd2, idx1, idx2, grad1, grad2, nblk1, nblk2, lay1, lay2, GS, PcmRescale());
    return pcm_launch_status();
}

// The backward of a one-launch step whose upstream gradient was not known when
// it ran (chamfer_bwd_slots_kernel's rescale mode): a no-op launch when
// *grad_loss equals *scale_used bit for bit, else the exact gradients of
// *grad_loss * (w1 sum(dist1) + w2 sum(dist2)) into gradxyz1/2 (their clouds'
// layouts); *scale_next = *grad_loss either way.  scale_used nullptr: always
// recompute.
extern "C" int pcm_chamfer_loss_grad_rescale(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1,
                                             int layout2, float w1, float w2, const float *grad_loss,
                                             const float *scale_used, float *scale_next, const int32_t *idx1,
                                             const int32_t *idx2, float *gradxyz1, float *gradxyz2, void *stream) {
    if (b <= 0 || n <= 0 || m <= 0 || (unsigned)layout1 > 1u || (unsigned)layout2 > 1u) return PCM_ERR_INVALID_ARG;
    if (n > kBwdSlotsMax || m > kBwdSlotsMax) return PCM_ERR_UNSUPPORTED;
    if (!xyz1 || !xyz2 || !grad_loss || !idx1 || !idx2 || !gradxyz1 || !gradxyz2) return PCM_ERR_INVALID_ARG;
    if (scale_next && (scale_next == grad_loss || scale_next == scale_used)) return PCM_ERR_INVALID_ARG;
    const int nblk1 = (n + kBwdSlotsT - 1) / kBwdSlotsT, nblk2 = (m + kBwdSlotsT - 1) / kBwdSlotsT;
    const long long blocks = (long long)b * (nblk1 + nblk2);
    if (blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    PcmRescale RS;
    RS.gl = grad_loss;
    RS.used = scale_used;
    RS.next = scale_next;
    RS.inv1 = w1;
    RS.inv2 = w2;
    const unsigned grid = (unsigned)(blocks < kRescaleGrid ? blocks : kRescaleGrid);
    hipLaunchKernelGGL(chamfer_bwd_slots_kernel, dim3(grid), dim3(kBwdSlotsT), 0, (hipStream_t)stream,
                       xyz1, xyz2, b, n, m, nullptr, nullptr, idx1, idx2, gradxyz1, gradxyz2, nblk1, nblk2, layout1,
                       layout2, PcmGdStr(), RS);
    return pcm_launch_status();
}

#define PCM_FWD_FILT(W, Q, C, TILE)                                                                   \
    PcmFwdVariant{chamfer_fwd_filt_kernel<float, W, Q, C, TILE, 0>, nullptr, nullptr,                \
                  chamfer_fwd_filt_kernel<float, W, Q, C, TILE, 3>, W, Q, false}
const PcmFwdVariant kPcmFiltVariants[] = {
    PCM_FWD_FILT(8, 2, 16, 2048),   // base + 0
    PCM_FWD_FILT(8, 4, 16, 2048),   // base + 1
    PCM_FWD_FILT(16, 4, 16, 2048),  // base + 2
    PCM_FWD_FILT(8, 4, 32, 2048),   // base + 3
    PCM_FWD_FILT(4, 4, 16, 2048),   // base + 4
    PCM_FWD_FILT(16, 2, 16, 2048),  // base + 5
    PCM_FWD_FILT(8, 4, 16, 4096),   // base + 6
    PCM_FWD_FILT(8, 8, 16, 2048),   // base + 7
    PCM_FWD_FILT(8, 4, 16, 1024),   // base + 8: the one-launch step's geometry (fused variant 11)
};
const int kPcmNumFiltVariants = sizeof(kPcmFiltVariants) / sizeof(kPcmFiltVariants[0]);

// fp16 clouds: coordinates widened on load (exact), then the same computation
const PcmFwd16Variant kPcmFilt16Variants[] = {
    {chamfer_fwd_filt_kernel<pcm_h, 8, 2, 16, 2048, 0>, 8, 2},  // f16 base + 0
    {chamfer_fwd_filt_kernel<pcm_h, 8, 4, 32, 2048, 0>, 8, 4},  // f16 base + 1
};
const int kPcmNumFilt16Variants = sizeof(kPcmFilt16Variants) / sizeof(kPcmFilt16Variants[0]);

// ---- fused loss + gradient: variants (tools/tune_chamfer.py) and entry points
namespace {
typedef void (*grad_kernel_t)(const float *, const float *, int, int, int, float, float, float *, float *,
                              int32_t *, int32_t *, float *, float *, float *, int, int, GradWs, unsigned,
                              unsigned, const float *);
struct GradVariant {
    int id;  // the variant number tools and tests name
    grad_kernel_t k;
    int waves, qpt;
};
// round 6: variant 7 (8-byte {tag, idx} argmin granules, both clouds copied
// into LDS for the gradient phase) again.  Round 5 had made 15 the default
// (4-byte granules, four per 16-byte write-through store, the gradient phase
// on the forward's own LDS: 3.09 MB of HBM-side traffic per launch against
// 3.65 MB) at the same time as 11; re-measured on the round-6 code, 7 is the
// fastest in every state: 13.09-13.12 vs 13.44-13.49 us in tools/ab_chamfer.py
// and 15.48-15.72 vs 15.79-15.99 us per step in the bench's own command
// (profiles/r06/bench_variants_r06zk_zl.txt)
// Since then: variant 19, 7's hand-off and gradient phase behind the
// matrix-core screen (filt_forward_mfma), for every size the entry takes
// (n, m <= 1024): 12.4 against 13.65 us in tools/ab_chamfer.py, the bench's
// own figures in DESIGN.md section 3.5c (profiles/mfma_screen/).
// Then variant 20, 19 with the wide screen loop (chained 32x32x16 MFMA pairs,
// filt_forward_mfma<.., true>): 11.2 against 11.7 us in tools/ab_chamfer.py
// (profiles/wide_screen/).
constexpr int kDefaultGradVariant = 20;
#define PCM_GRAD_DEFAULT_FORM(L1, L2, ONE) \
    chamfer_loss_grad_kernel<8, 4, 16, 1024, true, true, false, false, false, false, false, L1, L2, ONE, false, true>
#define PCM_GRAD_DEFAULT(L1, L2) PCM_GRAD_DEFAULT_FORM(L1, L2, false)
// The product library holds the default only; the measured alternatives are
// compiled into the tuning build (make tune: -DPCM_TUNE, libpcm_hip_tune.so),
// which tools/ and the variant tests load.
const GradVariant kGradVariants[] = {
#ifdef PCM_TUNE
    {0, chamfer_loss_grad_kernel<8, 2, 16, 1024>, 8, 2},
    {1, chamfer_loss_grad_kernel<8, 4, 16, 1024>, 8, 4},
    {2, chamfer_loss_grad_kernel<4, 2, 16, 1024>, 4, 2},
    {3, chamfer_loss_grad_kernel<16, 4, 16, 1024>, 16, 4},
    {4, chamfer_loss_grad_kernel<8, 4, 32, 1024>, 8, 4},
    {5, chamfer_loss_grad_kernel<16, 4, 32, 1024>, 16, 4},
    {6, chamfer_loss_grad_kernel<8, 4, 16, 1024, true>, 8, 4},  // screen on the matrix cores
    // 7: the granule hand-off behind the VALU screen (filt_forward); the default until 19
    {7, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true>, 8, 4},
    {8, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, true>, 8, 4},  // 7 + the clouds copied during the scan
    {9, chamfer_loss_grad_kernel<8, 4, 8, 1024, false, true>, 8, 4},   // 7 with 8-candidate chunks
    {10, chamfer_loss_grad_kernel<8, 4, 32, 1024, false, true>, 8, 4},  // 7 with 32-candidate chunks
    // 11: 7 whose gradient phase copies nothing in: the other cloud is the
    // forward's resident target tile, the range's points its queries
    {11, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, false, true>, 8, 4},
    // 12: 11 with the target tile staged and scanned in two halves
    {12, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, false, true, true>, 8, 4},
    // 13: LDS grid per workgroup (chamfer_lgrid.h): each group of 64 spatially
    // sorted queries screens only the target cells around it
    {13, chamfer_loss_grad_lgrid_kernel, 8, 4},
    // 14: 11 with 4-byte argmin granules and the range's own argmins taken
    // from the forward (half the hand-off bytes, no own-range granule reads)
    {14, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, false, true, false, true>, 8, 4},
    // 15: 14 with four granules per 16-byte write-through store (a quarter of
    // the fabric writes; the round-5 default)
    {15, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, false, true, false, true, true>, 8, 4},
    // 16: 7 (both clouds copied into LDS for the gradient phase) with 15's
    // granule hand-off: 4-byte granules, four per 16-byte store, the range's
    // own argmins from its forward
    {16, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, false, false, false, true, true>, 8, 4},
    // 17: 16 with one 4-byte granule store per query lane (no gathering shuffles)
    {17, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, false, false, false, true, false>, 8, 4},
    // 18: 7 with the range's own argmins from its forward (8-byte granules, no
    // own-range granule reads)
    {18, chamfer_loss_grad_kernel<8, 4, 16, 1024, false, true, false, false, false, false, false, 0, 0, false, true>, 8, 4},
    // 19: 7's hand-off and gradient phase behind the matrix-core screen (filt_forward_mfma); the default until 20
    {19, chamfer_loss_grad_kernel<8, 4, 16, 1024, true, true>, 8, 4},
#endif
    // 20 (the default): 19 with the wide screen loop (chained 32x32x16 MFMA pairs, filt_forward_mfma<.., true>)
    {kDefaultGradVariant, PCM_GRAD_DEFAULT(0, 0), 8, 4},
};
// the default variant with cloud 1 / cloud 2 in channel planes (index 2 lay1 + lay2)
const grad_kernel_t kGradDefaultLay[4] = {PCM_GRAD_DEFAULT(0, 0), PCM_GRAD_DEFAULT(0, 1), PCM_GRAD_DEFAULT(1, 0),
                                          PCM_GRAD_DEFAULT(1, 1)};
#ifdef PCM_TUNE
// the mixed-layout instances with one inlined forward (strides in registers):
// the matrix-core forward is always inlined once, so kLayOne changes nothing
// in it and the instances stay only so that lay_form 1 keeps its meaning
const grad_kernel_t kGradLayOne[4] = {
    PCM_GRAD_DEFAULT(0, 0),
    PCM_GRAD_DEFAULT_FORM(0, 1, true),
    PCM_GRAD_DEFAULT_FORM(1, 0, true),
    PCM_GRAD_DEFAULT(1, 1)};
#endif
#undef PCM_GRAD_DEFAULT
#undef PCM_GRAD_DEFAULT_FORM
// (round 5, rejected: 15 with two queries per lane -- 128-query workgroups,
// two per CU, four waves per SIMD -- 15.45 us against 13.39 us,
// profiles/r05/ab_qpt2_r05t.txt)
// (round 4, rejected: 7 and 11 with 16 waves -- four per SIMD, a 16-way
// merge -- 15.9-16.2 us against 13.85 us, profiles/r04/chamfer_w16_r04n_ab.txt)
// (round 4, rejected: 7 with the raw target rows parked in an LDS region of
// their own while staging, one barrier after the scan instead of two -- 13.28
// against 13.16 us, profiles/r04/chamfer_sept_r04q_ab.txt)
constexpr int kNumGradVariants = sizeof(kGradVariants) / sizeof(kGradVariants[0]);
constexpr int kMaxTuneVariantId = 20;  // the highest id of the tuning build's table above
// tools/tune_chamfer.py (profiles/r01): B=32, N=M=1024 -- W=8 QPT=4 18.7 us,
// W=8 QPT=2 19.3 us, W=4 QPT=2 21.4 us; round 2: variant 1 (arrival counter
// hand-off) 16.25 us, variant 7 (the same forward, granule hand-off) 14.97 us
// end of round 4 (after the latency-chain changes): variant 11, the same
// forward with the gradient phase reading the forward's own LDS instead of
// copying both clouds in, 0.07-0.12 us faster than 7 in each of 4 same-box
// runs (profiles/r04/variant_7_11_r04ze_ab.txt)

const GradVariant *find_grad_variant(int id) {
    for (int i = 0; i < kNumGradVariants; ++i)
        if (kGradVariants[i].id == id) return &kGradVariants[i];
    return nullptr;
}

long long grad_blocks(const GradVariant &v, int b, int n, int m, int &nblk1, int &nblk2) {
    const int QW = 64 * v.qpt;
    nblk1 = (n + QW - 1) / QW;
    nblk2 = (m + QW - 1) / QW;
    return (long long)b * (nblk1 + nblk2);
}

// the workspace serves every variant this build holds (the product build: the
// default alone)
long long grad_blocks_max(int b, int n, int m) {
    long long most = 0;
    for (int i = 0; i < kNumGradVariants; ++i) {
        int n1, n2;
        const long long bl = grad_blocks(kGradVariants[i], b, n, m, n1, n2);
        most = bl > most ? bl : most;
    }
    return most;
}

// the matrix-core forward takes single-tile clouds (n, m <= kMfmaTile): that is
// the entry's own limit (kGradCap, checked by launch_loss_grad), so 20 serves
// every size the entry accepts
static_assert(kMfmaTile >= kGradCap, "the default serves every size the entry takes");
int default_grad_variant(int, int, int) { return kDefaultGradVariant; }

int launch_loss_grad(int variant, const float *xyz1, const float *xyz2, int b, int n, int m, float w1, float w2,
                     float *dist1, float *dist2, int32_t *idx1, int32_t *idx2, float *mean_out, float *grad1,
                     float *grad2, void *workspace, size_t workspace_bytes, void *stream,
                     unsigned max_spins = kGradWaitSpins, unsigned poll_spins = pcm_loss::kPollMaxSpins,
                     int lay1 = 0, int lay2 = 0, const float *gscale = nullptr, int lay_form = 0) {
    if (b <= 0 || n <= 0 || m <= 0) return PCM_ERR_INVALID_ARG;
    if (n > kGradCap || m > kGradCap) return PCM_ERR_UNSUPPORTED;
    if ((unsigned)lay1 > 1u || (unsigned)lay2 > 1u) return PCM_ERR_INVALID_ARG;
    const GradVariant *v = find_grad_variant(variant);
    // a known id this build does not hold (all but the default: tuning build)
    if (!v) return variant >= 0 && variant <= kMaxTuneVariantId ? PCM_ERR_UNSUPPORTED : PCM_ERR_INVALID_ARG;
    if ((lay1 | lay2) && variant != kDefaultGradVariant) return PCM_ERR_UNSUPPORTED;
    if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2 || !mean_out || !grad1 || !grad2 || !workspace)
        return PCM_ERR_INVALID_ARG;
    int nblk1, nblk2;
    const long long blocks = grad_blocks(*v, b, n, m, nblk1, nblk2);
    if (blocks > 0x7ffffffeLL) return PCM_ERR_UNSUPPORTED;
    const size_t off = pcm_chamfer_loss_ws_offset(b, n, m);
    if (workspace_bytes < off + grad_ws_bytes(b, grad_blocks_max(b, n, m), (long long)b * (n + m)))
        return PCM_ERR_WORKSPACE;
    const GradWs ws = grad_ws((char *)workspace + off, b, blocks);
    grad_kernel_t k = variant == kDefaultGradVariant ? kGradDefaultLay[2 * lay1 + lay2] : v->k;
#ifdef PCM_TUNE
    if (lay_form == 1 && variant == kDefaultGradVariant) k = kGradLayOne[2 * lay1 + lay2];
#else
    if (lay_form != 0) return PCM_ERR_UNSUPPORTED;
#endif
    // + the polling workgroup (the grid's last)
    hipLaunchKernelGGL(k, dim3((unsigned)blocks + 1), dim3(64 * v->waves), 0, (hipStream_t)stream, xyz1, xyz2, b,
                       n, m, w1, w2, dist1, dist2, idx1, idx2, mean_out, grad1, grad2, nblk1, nblk2, ws, max_spins,
                       poll_spins, gscale);
    return pcm_launch_status();
}
}  // namespace

int pcm_chamfer_grad_err_word(void) { return kGradErrWord; }

size_t pcm_chamfer_grad_ws_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return grad_ws_bytes(b, grad_blocks_max(b, n, m), (long long)b * (n + m));
}

extern "C" int pcm_chamfer_loss_grad(const float *xyz1, const float *xyz2, int b, int n, int m, float w1,
                                     float w2, float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                                     float *mean_out, float *gradxyz1, float *gradxyz2, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return launch_loss_grad(default_grad_variant(b, n, m), xyz1, xyz2, b, n, m, w1, w2, dist1, dist2, idx1, idx2, mean_out,
                            gradxyz1, gradxyz2, workspace, workspace_bytes, stream);
}

extern "C" int pcm_chamfer_loss_grad_layout(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1,
                                            int layout2, float w1, float w2, const float *grad_scale, float *dist1,
                                            float *dist2, int32_t *idx1, int32_t *idx2, float *mean_out,
                                            float *gradxyz1, float *gradxyz2, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    return launch_loss_grad(default_grad_variant(b, n, m), xyz1, xyz2, b, n, m, w1, w2, dist1, dist2, idx1, idx2,
                            mean_out, gradxyz1, gradxyz2, workspace, workspace_bytes, stream, kGradWaitSpins,
                            pcm_loss::kPollMaxSpins, layout1, layout2, grad_scale);
}

// the layout entry with a chosen form of the mixed-layout instances (0: the
// product's two inlined forwards, 1: one forward with runtime strides; the
// tuning build only): tools/ab_layout_forms.py
extern "C" int pcm_tune_chamfer_loss_grad_layout(int form, const float *xyz1, const float *xyz2, int b, int n, int m,
                                                 int layout1, int layout2, float w1, float w2,
                                                 const float *grad_scale, float *dist1, float *dist2, int32_t *idx1,
                                                 int32_t *idx2, float *mean_out, float *gradxyz1, float *gradxyz2,
                                                 void *workspace, size_t workspace_bytes, void *stream) {
    return launch_loss_grad(default_grad_variant(b, n, m), xyz1, xyz2, b, n, m, w1, w2, dist1, dist2, idx1, idx2,
                            mean_out, gradxyz1, gradxyz2, workspace, workspace_bytes, stream, kGradWaitSpins,
                            pcm_loss::kPollMaxSpins, layout1, layout2, grad_scale, form);
}

// `steps` back-to-back launches of the default step from one host call, its
// arguments bound once: K steps of a native training loop on fixed buffers
// (what bench.py's N=1 region times; a ctypes call per step from Python is
// host-bound, ~17 us for 17 arguments against a ~14 us kernel)
extern "C" int pcm_chamfer_loss_grad_steps(int steps, const float *xyz1, const float *xyz2, int b, int n, int m,
                                           float w1, float w2, float *dist1, float *dist2, int32_t *idx1,
                                           int32_t *idx2, float *mean_out, float *gradxyz1, float *gradxyz2,
                                           void *workspace, size_t workspace_bytes, void *stream) {
    if (steps < 0) return PCM_ERR_INVALID_ARG;
    for (int r = 0; r < steps; ++r) {
        const int st = launch_loss_grad(default_grad_variant(b, n, m), xyz1, xyz2, b, n, m, w1, w2, dist1, dist2, idx1,
                                        idx2, mean_out, gradxyz1, gradxyz2, workspace, workspace_bytes, stream);
        if (st != PCM_OK) return st;
    }
    return PCM_OK;
}

extern "C" int pcm_tune_chamfer_loss_grad(int variant, const float *xyz1, const float *xyz2, int b, int n, int m,
                                          float w1, float w2, float *dist1, float *dist2, int32_t *idx1,
                                          int32_t *idx2, float *mean_out, float *gradxyz1, float *gradxyz2,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    return launch_loss_grad(variant, xyz1, xyz2, b, n, m, w1, w2, dist1, dist2, idx1, idx2, mean_out, gradxyz1,
                            gradxyz2, workspace, workspace_bytes, stream);
}

// variants this build holds (the product: the default alone)
extern "C" int pcm_tune_num_chamfer_loss_grad_variants(void) { return kNumGradVariants; }

namespace {
// variant 0: the filtered geometry of larger clouds (W 8, QPT 4, C 32, 2048-point tiles); 1: that of clouds of
// <= 1024 points and of the one-launch step (C 16, 1024-point tiles), as chamfer.hip default_fwd_variant picks
int launch_fwd_layout(int variant, const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                      float *dist1, float *dist2, int32_t *idx1, int32_t *idx2, void *stream) {
    if (b < 0 || n < 0 || m < 0 || (unsigned)layout1 > 1u || (unsigned)layout2 > 1u || (unsigned)variant > 1u)
        return PCM_ERR_INVALID_ARG;
    if (layout1 == 0 && layout2 == 0 && variant == 0)
        return pcm_chamfer_forward(xyz1, xyz2, b, n, m, dist1, dist2, idx1, idx2, stream);
    if (b == 0 || (n == 0 && m == 0)) return PCM_OK;
    if ((n > 0 && (!xyz1 || !dist1 || !idx1)) || (m > 0 && (!xyz2 || !dist2 || !idx2))) return PCM_ERR_INVALID_ARG;
    constexpr int W = 8, QPT = 4, QW = 64 * QPT;
    const int nblk1 = m > 0 ? (n + QW - 1) / QW : 0;  // a direction without targets keeps its outputs
    const int nblk2 = n > 0 ? (m + QW - 1) / QW : 0;
    const long long blocks = (long long)b * (nblk1 + nblk2);
    if (blocks > 0x7ffffffeLL) return PCM_ERR_UNSUPPORTED;
    if (blocks == 0) return PCM_OK;
    typedef void (*lay_kernel_t)(const float *, const float *, int, int, int, float *, float *, int32_t *, int32_t *,
                                 int, int);
    static const lay_kernel_t k32[4] = {
        chamfer_fwd_filt_lay_kernel<W, QPT, 32, 2048, 0, 0>, chamfer_fwd_filt_lay_kernel<W, QPT, 32, 2048, 0, 1>,
        chamfer_fwd_filt_lay_kernel<W, QPT, 32, 2048, 1, 0>, chamfer_fwd_filt_lay_kernel<W, QPT, 32, 2048, 1, 1>};
    static const lay_kernel_t k16[4] = {
        chamfer_fwd_filt_lay_kernel<W, QPT, 16, 1024, 0, 0>, chamfer_fwd_filt_lay_kernel<W, QPT, 16, 1024, 0, 1>,
        chamfer_fwd_filt_lay_kernel<W, QPT, 16, 1024, 1, 0>, chamfer_fwd_filt_lay_kernel<W, QPT, 16, 1024, 1, 1>};
    const lay_kernel_t k = (variant == 0 ? k32 : k16)[2 * layout1 + layout2];
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * W), 0, (hipStream_t)stream, xyz1, xyz2, b, n, m, dist1,
                       dist2, idx1, idx2, nblk1, nblk2);
    return pcm_launch_status();
}
}  // namespace

extern "C" int pcm_chamfer_forward_layout(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1,
                                          int layout2, float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                                          void *stream) {
    // the geometry chamfer.hip default_fwd_variant picks for the rows
    const int v = (n <= 1024 && m <= 1024) ? 1 : 0;
    if (layout1 == 0 && layout2 == 0) return pcm_chamfer_forward(xyz1, xyz2, b, n, m, dist1, dist2, idx1, idx2, stream);
    return launch_fwd_layout(v, xyz1, xyz2, b, n, m, layout1, layout2, dist1, dist2, idx1, idx2, stream);
}

extern "C" int pcm_tune_chamfer_forward_layout(int variant, const float *xyz1, const float *xyz2, int b, int n, int m,
                                               int layout1, int layout2, float *dist1, float *dist2, int32_t *idx1,
                                               int32_t *idx2, void *stream) {
    return launch_fwd_layout(variant, xyz1, xyz2, b, n, m, layout1, layout2, dist1, dist2, idx1, idx2, stream);
}

// the default variant with given bounds on the gradient-phase waits
// (wait_spins; 0: every argmin recomputed locally, exact results) and on the
// loss poll (poll_spins; 0 forces its timeout: sticky error word, NaN means)
extern "C" int pcm_tune_chamfer_loss_grad_spins(unsigned wait_spins, unsigned poll_spins, const float *xyz1,
                                                const float *xyz2, int b, int n, int m, float w1, float w2,
                                                float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                                                float *mean_out, float *gradxyz1, float *gradxyz2, void *workspace,
                                                size_t workspace_bytes, void *stream) {
    return launch_loss_grad(default_grad_variant(b, n, m), xyz1, xyz2, b, n, m, w1, w2, dist1, dist2, idx1, idx2, mean_out,
                            gradxyz1, gradxyz2, workspace, workspace_bytes, stream, wait_spins, poll_spins);
}

// diagnostics: gradient-phase waits on `workspace` that timed out and computed
// the missing argmins locally, summed over every call since it was zero-filled
// (>= 0, or a negative pcm_status); synchronises `stream`
extern "C" int pcm_tune_chamfer_slow_paths(const void *workspace, size_t workspace_bytes, int b, int n, int m,
                                           void *stream) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    if (!workspace || workspace_bytes < pcm_chamfer_loss_ws_offset(b, n, m) + pcm_chamfer_grad_ws_bytes(b, n, m))
        return PCM_ERR_WORKSPACE;
    unsigned v = 0;
    const char *p = (const char *)workspace + pcm_chamfer_loss_ws_offset(b, n, m) + 4 * kGradSlowWord;
    if (hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return PCM_ERR_LAUNCH;
    return (int)(v & 0x7fffffffu);
}

#ifdef PCM_STAMPS
extern "C" int pcm_tune_read_stamps(unsigned long long *host, int nblocks) {
    if (nblocks > kStampSlots) nblocks = kStampSlots;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pcm_stamps), (size_t)nblocks * 8 * 8, 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? nblocks : -1;
}
#endif

#ifdef PCM_STAMPS
// Core clock estimate (profiling build): every workgroup spins ~20 us of
// dependent VALU work between two (s_memtime, s_memrealtime) pairs.
__global__ void pcm_clock_kernel(unsigned long long *out, int iters) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    float v = (float)threadIdx.x;
    for (int i = 0; i < iters; ++i) v = __builtin_fmaf(v, 0.999f, 0.5f);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        out[4 * blockIdx.x + 0] = t1 - t0;
        out[4 * blockIdx.x + 1] = r1 - r0;
        out[4 * blockIdx.x + 2] = __float_as_uint(v);
    }
}
extern "C" int pcm_tune_clock(unsigned long long *dev_out, int blocks, int iters, void *stream) {
    hipLaunchKernelGGL(pcm_clock_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dev_out, iters);
    return pcm_launch_status();
}
#endif
