// sinkhorn.hip -- debiased Sinkhorn divergence of two uniformly weighted clouds
// for MI355X (gfx950, CDNA4): the symmetric, averaged Sinkhorn loop with
// epsilon-scaling and a last extrapolation step that also gives both
// gradients.  include/pcm.h has the contract; DESIGN.md section 3.17 has the
// rationale and the numbers.  The algorithm is geomloss's published one
// (sinkhorn_loop); geomloss is not installed here, so it is NOT verified
// against that package (include/pcm.h says the same).
//
// T + 3 launches for a schedule of T entries, all deterministic:
//   1. sinkhorn_step (T + 1 launches: the initialisation, then one a schedule
//      entry).  kernel_loss.hip's scan: a workgroup of eight waves owns
//      kSkRows = 128 points ("rows") of ONE cloud of one element, two to a
//      lane; the columns -- first the rows' own cloud, then the other one -- go
//      through an LDS tile of kSkTile = 1024 points packed (x, y, z, h), h the
//      column's log2-weight plus its potential scaled by log2(e) / eps, formed
//      once when the tile is staged.  Own-cloud tiles carry the symmetric
//      potential, other-cloud tiles the cross one.  Wave w takes the w-th
//      eighth of every tile in groups of kSkGroup = 4 columns: the group's
//      exponents t = fmaf(d2, c, h), their maximum with the running one, a
//      rescale of the running sum only where some lane's maximum rose (a
//      wave-uniform branch; the factor is exp2(0) = 1 exactly for the lanes
//      whose maximum stayed, so the bits do not depend on the branch), then
//      one hardware exp2 and one add a pair.  The waves' (max, sum) pairs meet in
//      LDS (the tile's storage) and wave 0 merges them in ascending wave order
//      and writes the row's two potentials to the other half of the workspace.
//   2. sinkhorn_step<true>: the extrapolation.  The same scan; a cloud with a
//      gradient pointer also carries sum w (p - q) in three more accumulators
//      a softmin under the same rescaling and writes its gradient.
//   3. sinkhorn_finish: one workgroup an element adds the rows' terms in
//      double in kernel_loss_finish's fixed order and rounds once.
// No atomics, no waiting between workgroups, nothing kept in the workspace.
#include <math.h>

#include "pcm_common.h"

namespace {

constexpr int kSkMaxN = PCM_SINKHORN_MAX_POINTS;
constexpr int kSkWaves = 8;                  // waves per workgroup: each an eighth of every tile
constexpr int kSkThreads = 64 * kSkWaves;
constexpr int kSkPerLane = 2;                // rows per lane
constexpr int kSkRows = 64 * kSkPerLane;     // rows per workgroup
constexpr int kSkTile = 1024;                // column points per LDS tile (16 KiB)
constexpr int kSkShare = kSkTile / kSkWaves;
constexpr int kSkGroup = 4;                  // columns whose maximum is taken together
constexpr int kSkFinishThreads = 256;

// float4 slots of the workgroup's LDS: the tile, or the accumulators of waves 1.. that take its place at
// the end (four a row: 14 KiB; ten with gradients: 35 KiB), whichever is more
constexpr int sk_shared(bool grad) {
    const int merge = (kSkWaves - 1) * (grad ? 10 : 4) * kSkRows / 4;
    return merge > kSkTile ? merge : kSkTile;
}

struct SkStep {
    float c;         // fl(-log2(e) / (2 eps)): the exponent of a pair is fmaf(d2, c, h)
    float s;         // fl(log2(e) / eps): a column's h = fmaf(potential, s, log2 weight)
    float out;       // fl(-eps ln 2): a softmin is (max + log2 sum) * out
    float lw1, lw2;  // fl(-log2 n), fl(-log2 m)
    int mode;        // 0: initialisation (no potentials read), 1: averaged update, 2: extrapolation
};

// One running softmin of a row: the maximum M of the exponents seen, S = sum 2^(t - M) and, with
// gradients, A = sum 2^(t - M) (p - q)
struct SkAcc {
    float M[kSkPerLane], S[kSkPerLane], A[kSkPerLane][3];
};

// G columns from q on of the tile against both rows of the lane
template <int G, bool GRAD>
__device__ __forceinline__ void sk_group(const pcm_f4 *sTile, int q, float c, const float (&px)[kSkPerLane],
                                         const float (&py)[kSkPerLane], const float (&pz)[kSkPerLane],
                                         SkAcc &acc) {
    pcm_f4 v[G];
#pragma unroll
    for (int g = 0; g < G; ++g) v[g] = sTile[q + g];
#pragma unroll
    for (int r = 0; r < kSkPerLane; ++r) {
        float dx[G], dy[G], dz[G], t[G];
        float nm = acc.M[r];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            dx[g] = px[r] - v[g].x;
            dy[g] = py[r] - v[g].y;
            dz[g] = pz[r] - v[g].z;
            t[g] = __builtin_fmaf(pcm_sqd(dx[g], dy[g], dz[g]), c, v[g].w);
            nm = __builtin_fmaxf(nm, t[g]);
        }
        if (__builtin_amdgcn_ballot_w64(nm > acc.M[r]) != 0ull) {  // wave-uniform; a factor of exactly 1 elsewhere
            asm volatile("");  // or the compiler computes the factor always and selects
            const float sc = __builtin_amdgcn_exp2f(acc.M[r] - nm);
            acc.S[r] *= sc;
            if constexpr (GRAD) {
                acc.A[r][0] *= sc;
                acc.A[r][1] *= sc;
                acc.A[r][2] *= sc;
            }
        }
        acc.M[r] = nm;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float w = __builtin_amdgcn_exp2f(t[g] - nm);
            acc.S[r] += w;
            if constexpr (GRAD) {
                acc.A[r][0] = __builtin_fmaf(w, dx[g], acc.A[r][0]);
                acc.A[r][1] = __builtin_fmaf(w, dy[g], acc.A[r][1]);
                acc.A[r][2] = __builtin_fmaf(w, dz[g], acc.A[r][2]);
            }
        }
    }
}

// The rows' softmin against the cloud Q of `cnt` points: this wave's share of every tile, ascending, in
// groups of kSkGroup and then single columns.  pot: the (cross, own) potentials of Q's points, component
// `comp` of which enters h (not read when init).  Full workgroup, uniform control flow.
template <bool GRAD>
__device__ __forceinline__ void sk_scan(const float *__restrict__ Q, PcmLay L, int cnt,
                                        const float2 *__restrict__ pot, int comp, bool init, float s, float lw,
                                        float c, int wave, const float (&px)[kSkPerLane],
                                        const float (&py)[kSkPerLane], const float (&pz)[kSkPerLane], SkAcc &acc,
                                        pcm_f4 *sTile) {
    for (int t0 = 0; t0 < cnt; t0 += kSkTile) {
        __syncthreads();  // the previous tile has been read
        const int cntT = min(kSkTile, cnt - t0);
        for (int p = threadIdx.x; p < cntT; p += kSkThreads) {  // a full tile is two points a thread
            pcm_f4 v;
            v.x = Q[pcm_at(L, t0 + p, 0)];
            v.y = Q[pcm_at(L, t0 + p, 1)];
            v.z = Q[pcm_at(L, t0 + p, 2)];
            v.w = lw;
            if (!init) {
                const float2 f = pot[t0 + p];
                v.w = __builtin_fmaf(comp ? f.y : f.x, s, lw);
            }
            sTile[p] = v;
        }
        __syncthreads();
        const int beg = wave * kSkShare, end = min(cntT, (wave + 1) * kSkShare);
        int q = beg;
#pragma unroll 2
        for (; q + kSkGroup <= end; q += kSkGroup) sk_group<kSkGroup, GRAD>(sTile, q, c, px, py, pz, acc);
        for (; q < end; ++q) sk_group<1, GRAD>(sTile, q, c, px, py, pz, acc);
    }
}

__device__ __forceinline__ void sk_clear(SkAcc &a) {
#pragma unroll
    for (int r = 0; r < kSkPerLane; ++r) {
        a.M[r] = -PCM_INF;
        a.S[r] = 0.f;
        a.A[r][0] = a.A[r][1] = a.A[r][2] = 0.f;
    }
}

// Rows blk * kSkRows .. of the cloud `own` (no points, log2 weight lwo; the other cloud `oth`: nt, lwt):
// the two scans, the waves' merge and the outputs.  oldOwn / oldOth: the clouds' (cross, own) potentials
// this step reads; newOwn: where the rows' new ones go; potOut: the caller's copy (or null); G: the own
// cloud's gradient of this element (GRAD), w its points' weight.
template <bool GRAD>
__device__ __forceinline__ void sk_block(const float *__restrict__ own, PcmLay Lo, int no, float lwo,
                                         const float *__restrict__ oth, PcmLay Lt, int nt, float lwt, int blk,
                                         const SkStep &st, const float2 *__restrict__ oldOwn,
                                         const float2 *__restrict__ oldOth, float2 *__restrict__ newOwn,
                                         float2 *__restrict__ potOut, float *__restrict__ G, float w,
                                         pcm_f4 *sTile) {
    constexpr int NA = GRAD ? 10 : 4;  // accumulators per row: (M, S) own, (M, S) other, A own, A other
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool init = st.mode == 0;

    float px[kSkPerLane], py[kSkPerLane], pz[kSkPerLane];
#pragma unroll
    for (int r = 0; r < kSkPerLane; ++r) {
        const int i = blk * kSkRows + r * 64 + lane;
        const int at = i < no ? i : 0;  // a lane past the cloud scans point 0 and writes nothing
        px[r] = own[pcm_at(Lo, at, 0)];
        py[r] = own[pcm_at(Lo, at, 1)];
        pz[r] = own[pcm_at(Lo, at, 2)];
    }
    SkAcc a0, a1;
    sk_clear(a0);
    sk_clear(a1);
    sk_scan<GRAD>(own, Lo, no, oldOwn, 1, init, st.s, lwo, st.c, wave, px, py, pz, a0, sTile);
    sk_scan<GRAD>(oth, Lt, nt, oldOth, 0, init, st.s, lwt, st.c, wave, px, py, pz, a1, sTile);

    __syncthreads();  // the last tile has been read: its storage takes the accumulators of waves 1..
    float *sAcc = (float *)sTile;  // [wave - 1][accumulator][row of the workgroup]
#pragma unroll
    for (int r = 0; r < kSkPerLane; ++r) {
        const float a[10] = {a0.M[r], a0.S[r], a1.M[r], a1.S[r], a0.A[r][0], a0.A[r][1], a0.A[r][2],
                             a1.A[r][0], a1.A[r][1], a1.A[r][2]};
        if (wave > 0) {
#pragma unroll
            for (int k = 0; k < NA; ++k) sAcc[((wave - 1) * NA + k) * kSkRows + r * 64 + lane] = a[k];
        }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int r = 0; r < kSkPerLane; ++r) {
        float a[10] = {a0.M[r], a0.S[r], a1.M[r], a1.S[r], a0.A[r][0], a0.A[r][1], a0.A[r][2],
                       a1.A[r][0], a1.A[r][1], a1.A[r][2]};
#pragma unroll
        for (int wv = 0; wv < kSkWaves - 1; ++wv) {  // waves 1, 2, .. 7 into wave 0's, in that order
            float o[10];
#pragma unroll
            for (int k = 0; k < NA; ++k) o[k] = sAcc[(wv * NA + k) * kSkRows + r * 64 + lane];
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // own, other
                const float nm = __builtin_fmaxf(a[2 * h], o[2 * h]);
                const float fa = __builtin_amdgcn_exp2f(a[2 * h] - nm), fo = __builtin_amdgcn_exp2f(o[2 * h] - nm);
                a[2 * h] = nm;
                a[2 * h + 1] = a[2 * h + 1] * fa + o[2 * h + 1] * fo;
                if constexpr (GRAD) {
#pragma unroll
                    for (int k = 4 + 3 * h; k < 7 + 3 * h; ++k) a[k] = a[k] * fa + o[k] * fo;
                }
            }
        }
        const int i = blk * kSkRows + r * 64 + lane;
        if (i < no) {
            const float Fown = (a[0] + __builtin_amdgcn_logf(a[1])) * st.out;
            const float Fcross = (a[2] + __builtin_amdgcn_logf(a[3])) * st.out;
            float2 res = float2{Fcross, Fown};
            if (st.mode == 1) {
                const float2 old = oldOwn[i];
                res = float2{0.5f * (old.x + Fcross), 0.5f * (old.y + Fown)};
            }
            newOwn[i] = res;
            if (potOut) potOut[i] = res;
            if constexpr (GRAD) {
                G[pcm_at(Lo, i, 0)] = w * (a[7] / a[3] - a[4] / a[1]);
                G[pcm_at(Lo, i, 1)] = w * (a[8] / a[3] - a[5] / a[1]);
                G[pcm_at(Lo, i, 2)] = w * (a[9] / a[3] - a[6] / a[1]);
            }
        }
    }
}

// element bid / (nblk1 + nblk2): its nblk1 row blocks of cloud 1, then the nblk2 of cloud 2.
// EXTRAP: the extrapolation step (st.mode == 2), the only one that writes gradients and potentials_out.
template <bool EXTRAP>
__global__ __launch_bounds__(kSkThreads) void sinkhorn_step(const float *__restrict__ xyz1,
                                                            const float *__restrict__ xyz2, int n, int m,
                                                            int planes1, int planes2, int nblk1, int nblk2,
                                                            SkStep st, const float2 *__restrict__ potOld,
                                                            float2 *__restrict__ potNew,
                                                            float2 *__restrict__ potOut,
                                                            float *__restrict__ gradxyz1,
                                                            float *__restrict__ gradxyz2, float w1, float w2) {
    __shared__ pcm_f4 sTile[sk_shared(EXTRAP)];
    int bi, blk;
    bool first;
    pcm_split_bm(pcm_xcd_remap(blockIdx.x, gridDim.x), nblk1, nblk2, bi, first, blk);
    const float *P1 = xyz1 + (size_t)bi * n * 3, *P2 = xyz2 + (size_t)bi * m * 3;
    const PcmLay L1 = pcm_lay(planes1, n), L2 = pcm_lay(planes2, m);
    const size_t rows = (size_t)bi * ((size_t)n + m);
    const float2 *O1 = potOld + rows, *O2 = O1 + n;
    float2 *N1 = potNew + rows, *N2 = N1 + n;
    if constexpr (EXTRAP) {
        float2 *U1 = potOut ? potOut + rows : nullptr, *U2 = potOut ? U1 + n : nullptr;
        if (first) {
            float *G = gradxyz1 ? gradxyz1 + (size_t)bi * n * 3 : nullptr;
            if (G) sk_block<true>(P1, L1, n, st.lw1, P2, L2, m, st.lw2, blk, st, O1, O2, N1, U1, G, w1, sTile);
            else sk_block<false>(P1, L1, n, st.lw1, P2, L2, m, st.lw2, blk, st, O1, O2, N1, U1, G, w1, sTile);
        } else {
            float *G = gradxyz2 ? gradxyz2 + (size_t)bi * m * 3 : nullptr;
            if (G) sk_block<true>(P2, L2, m, st.lw2, P1, L1, n, st.lw1, blk, st, O2, O1, N2, U2, G, w2, sTile);
            else sk_block<false>(P2, L2, m, st.lw2, P1, L1, n, st.lw1, blk, st, O2, O1, N2, U2, G, w2, sTile);
        }
    } else {
        if (first) sk_block<false>(P1, L1, n, st.lw1, P2, L2, m, st.lw2, blk, st, O1, O2, N1, nullptr, nullptr, w1, sTile);
        else sk_block<false>(P2, L2, m, st.lw2, P1, L1, n, st.lw1, blk, st, O2, O1, N2, nullptr, nullptr, w2, sTile);
    }
}

// loss_out[blockIdx.x] from the element's rows' (F_cross, F_own), in double: thread t adds rows t, t + 256,
// .. ascending, every wave its 64 threads by the six DPP steps, thread 0 the four waves' sums ascending
__global__ __launch_bounds__(kSkFinishThreads) void sinkhorn_finish(const float2 *__restrict__ pot, int n, int m,
                                                                    float *__restrict__ loss_out) {
    __shared__ double sWave[kSkFinishThreads / 64];
    const int rows = n + m;
    const float2 *R = pot + (size_t)blockIdx.x * rows;
    const double a = 1.0 / (double)n, b = 1.0 / (double)m;
    double acc = 0.0;
    for (int r = threadIdx.x; r < rows; r += kSkFinishThreads) {
        const float2 f = R[r];
        acc += (r < n ? a : b) * ((double)f.x - (double)f.y);
    }
    const double wsum = pcm_wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) sWave[threadIdx.x >> 6] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < kSkFinishThreads / 64; ++w) total += sWave[w];
        loss_out[blockIdx.x] = (float)total;
    }
}

inline int sk_blocks(int n) { return (n + kSkRows - 1) / kSkRows; }

}  // namespace

extern "C" int pcm_sinkhorn_schedule(float blur, float scaling, float diameter, double *eps_out, int capacity) {
    if (!__builtin_isfinite(blur) || !__builtin_isfinite(scaling) || !__builtin_isfinite(diameter))
        return PCM_ERR_INVALID_ARG;
    if (!(blur > 0.f) || !(diameter > 0.f) || !(scaling > 0.f) || !(scaling < 1.f)) return PCM_ERR_INVALID_ARG;
    const double lo = 2.0 * log((double)blur), hi = 2.0 * log((double)diameter), step = 2.0 * log((double)scaling);
    int count = 1;  // eps_0
    for (int k = 1; hi + (double)(k - 1) * step > lo; ++k) {
        if (++count > PCM_SINKHORN_MAX_STEPS) return PCM_ERR_UNSUPPORTED;
    }
    if (++count > PCM_SINKHORN_MAX_STEPS) return PCM_ERR_UNSUPPORTED;  // blur^2
    if (eps_out && capacity >= count) {
        int at = 0;
        eps_out[at++] = (double)diameter * (double)diameter;
        for (int k = 1; hi + (double)(k - 1) * step > lo; ++k) eps_out[at++] = exp(hi + (double)(k - 1) * step);
        eps_out[at++] = (double)blur * (double)blur;
    }
    return count;
}

extern "C" size_t pcm_sinkhorn_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return 2 * (size_t)b * ((size_t)n + (size_t)m) * sizeof(float2);  // two halves of (cross, own) a point
}

extern "C" int pcm_sinkhorn_loss(const float *xyz1, const float *xyz2, int b, int n, int m, int layout1, int layout2,
                                 float blur, float scaling, float diameter, float *loss_out, float *gradxyz1,
                                 float *gradxyz2, float *potentials_out, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    if (b < 0 || n < 0 || m < 0) return PCM_ERR_INVALID_ARG;
    if ((layout1 != 0 && layout1 != 1) || (layout2 != 0 && layout2 != 1)) return PCM_ERR_INVALID_ARG;
    double eps[PCM_SINKHORN_MAX_STEPS];
    const int T = pcm_sinkhorn_schedule(blur, scaling, diameter, eps, PCM_SINKHORN_MAX_STEPS);
    if (T < 0) return T;
    if (b == 0) return PCM_OK;
    if (n == 0 || m == 0 || !xyz1 || !xyz2 || !loss_out) return PCM_ERR_INVALID_ARG;
    if (n > kSkMaxN || m > kSkMaxN) return PCM_ERR_UNSUPPORTED;
    if ((long long)b * (sk_blocks(n) + sk_blocks(m)) > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;  // the grid
    if (!workspace || workspace_bytes < pcm_sinkhorn_workspace_bytes(b, n, m)) return PCM_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return PCM_ERR_INVALID_ARG;

    const double log2e = 1.4426950408889634, ln2 = 0.6931471805599453;
    const int nblk1 = sk_blocks(n), nblk2 = sk_blocks(m);
    const dim3 grid((unsigned)(b * (nblk1 + nblk2))), block(kSkThreads);
    const float w1 = (float)(1.0 / (double)n), w2 = (float)(1.0 / (double)m);
    float2 *half[2] = {(float2 *)workspace, (float2 *)workspace + (size_t)b * ((size_t)n + m)};
    hipStream_t st = (hipStream_t)stream;
    SkStep p;
    p.lw1 = (float)(-log2((double)n));
    p.lw2 = (float)(-log2((double)m));
    auto at = [&](double e, int mode) {
        p.c = (float)(-log2e / (2.0 * e));
        p.s = (float)(log2e / e);
        p.out = (float)(-e * ln2);
        p.mode = mode;
    };
    int cur = 0;  // the half that holds the current potentials once the initialisation has run
    at(eps[0], 0);
    hipLaunchKernelGGL(sinkhorn_step<false>, grid, block, 0, st, xyz1, xyz2, n, m, layout1, layout2, nblk1, nblk2, p,
                       (const float2 *)half[1], half[0], (float2 *)nullptr, (float *)nullptr, (float *)nullptr, w1,
                       w2);
    for (int k = 0; k < T; ++k) {
        at(eps[k], 1);
        hipLaunchKernelGGL(sinkhorn_step<false>, grid, block, 0, st, xyz1, xyz2, n, m, layout1, layout2, nblk1, nblk2,
                           p, (const float2 *)half[cur], half[cur ^ 1], (float2 *)nullptr, (float *)nullptr,
                           (float *)nullptr, w1, w2);
        cur ^= 1;
    }
    at(eps[T - 1], 2);
    hipLaunchKernelGGL(sinkhorn_step<true>, grid, block, 0, st, xyz1, xyz2, n, m, layout1, layout2, nblk1, nblk2, p,
                       (const float2 *)half[cur], half[cur ^ 1], (float2 *)potentials_out, gradxyz1, gradxyz2, w1,
                       w2);
    hipLaunchKernelGGL(sinkhorn_finish, dim3((unsigned)b), dim3(kSkFinishThreads), 0, st,
                       (const float2 *)half[cur ^ 1], n, m, loss_out);
    return pcm_launch_status();
}
