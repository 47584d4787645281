// chamfer_eval.hip -- one-pass Chamfer evaluation for MI355X (gfx950, CDNA4):
// per-cloud F-score / precision / recall at up to eight squared-distance
// thresholds, and the per-cloud mean nearest-neighbour distances.
//
// Replaces, for an evaluation loop, batch_NN_loss + fscore of the reference's
// loss/loss_.py:93-109, :122-140 (a B x N x M float64 distance matrix, two
// min reductions, then compare / cast / mean / arithmetic / NaN fix-up per
// threshold).  DESIGN.md section 3.11 has the rationale and the measurements.
//
// Scan kernel: a workgroup owns 64*QPT query points of one (batch, direction)
// and W waves; the opposing cloud is staged through LDS in SoA tiles exactly as
// chamfer_fwd_kernel (chamfer.hip) stages it, and each wave scans an
// interleaved 1/W share of the tile's chunks, two candidates at a time in
// packed fp32 in the pinned order fma(dz,dz,fma(dy,dy,dx*dx)).  Only the
// running minimum is kept: for finite inputs the minimum of the pinned values
// does not depend on the scan order, so it IS the dist1/dist2 entry of
// pcm_chamfer_forward, and neither an argmin nor a rescan is needed (7 lane
// operations per pair against the argmin scan's 9).  A workgroup that sees a
// non-finite coordinate diverts to the reference-exact scan (pcm_ref_nn_scan),
// as the dense forward does, so NaN outcomes follow the 512-point tile rule.
// The epilogue runs one thread per query: threshold hits by ballot + popcount,
// the distance sum by a DPP wave sum; the workgroup stores ONE record
// {sum, count[0..8)} at its logical block slot.  Nothing per point is stored.
//
// Finalise kernel (one workgroup, next on the stream): the kernel boundary is
// the hand-off -- no tickets, no polling, no atomics.  It adds each cloud's
// records in ascending block order and writes every output.
#include "pcm_common.h"
#include "chamfer_loss.h"

using pcm_loss::wave_sum;

namespace {

constexpr int kEvalMaxTh = 8;              // thresholds per call
constexpr int kEvalRec = 1 + kEvalMaxTh;   // words per workgroup record: sum, counts
constexpr int kEvalTile = 2048;            // candidates per LDS tile (3 x 8 KiB SoA)
constexpr int kEvalChunk = 32;             // candidates per wave step
constexpr int kEvalW = 8;                  // waves per workgroup
constexpr int kEvalFinT = 256;             // threads of the finalise workgroup

// thresholds travel by value in the kernel arguments: no device buffer, so the
// call is capturable; slots past nth hold -inf (d < -inf never holds)
struct EvalTh {
    float v[kEvalMaxTh];
};

template <typename TIn, int W, int QPT, int C, int TILE>
__global__ __launch_bounds__(64 * W) void chamfer_eval_scan_kernel(
    const TIn *__restrict__ xyz1, const TIn *__restrict__ xyz2, int n, int m, int nblk1, int nblk2, EvalTh th,
    unsigned *__restrict__ records) {
    static_assert(TILE % C == 0 && C % 4 == 0, "tile must hold whole chunks");
    constexpr int QW = 64 * QPT;
    constexpr int NT = 64 * W;
    static_assert(QW <= NT, "one thread finalises one query");
    __shared__ __attribute__((aligned(16))) float sXYZ[3][TILE];
    __shared__ float sBest[W][QW];
    __shared__ int sNF[W];
    __shared__ float sSum[W];
    __shared__ int sCnt[W][kEvalMaxTh];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // ---- which (batch, direction, query block) this workgroup owns (uniform):
    // batch-major, so both directions of an element share an XCD and its L2
    const int slot = pcm_xcd_remap((int)blockIdx.x, (int)gridDim.x);  // logical block id = record index
    int batch, blk;
    bool first;
    pcm_split_bm(slot, nblk1, nblk2, batch, first, blk);
    const TIn *Q = first ? xyz1 + (size_t)batch * n * 3 : xyz2 + (size_t)batch * m * 3;
    const TIn *T = first ? xyz2 + (size_t)batch * m * 3 : xyz1 + (size_t)batch * n * 3;
    const int nq = first ? n : m;
    const int nt = first ? m : n;
    const int qbase = blk * QW;

    // ---- this lane's query points (splatted for the packed math)
    pcm_f2 px[QPT], py[QPT], pz[QPT];
    bool nonfinite = false;
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        const int qi = qbase + qq * 64 + lane;
        float x = 0.f, y = 0.f, z = 0.f;
        if (qi < nq) {
            x = pcm_ld(Q + 3 * (size_t)qi + 0);
            y = pcm_ld(Q + 3 * (size_t)qi + 1);
            z = pcm_ld(Q + 3 * (size_t)qi + 2);
            nonfinite |= !(pcm_finite(x) && pcm_finite(y) && pcm_finite(z));
        }
        px[qq] = pcm_f2{x, x};
        py[qq] = pcm_f2{y, y};
        pz[qq] = pcm_f2{z, z};
    }

    float best[QPT];
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) best[qq] = PCM_INF;

    for (int t0 = 0; t0 < nt; t0 += TILE) {
        const int cnt = min(TILE, nt - t0);
        const int padded = (cnt + C - 1) / C * C;
        if (t0 > 0) __syncthreads();  // previous tile fully consumed
        // coalesced flat read of the AoS tile, scattered to SoA; pad = +inf.
        // All of a thread's loads are issued before any LDS write, so the
        // tile costs one memory latency, not one per element.
        const TIn *src = T + 3 * (size_t)t0;
        constexpr int kFill = (3 * TILE + NT - 1) / NT;
        float v[kFill];
#pragma unroll
        for (int r = 0; r < kFill; ++r) {
            const int f = tid + r * NT;
            v[r] = (f < 3 * cnt) ? pcm_ld(src + f) : PCM_INF;
        }
#pragma unroll
        for (int r = 0; r < kFill; ++r) {
            const int f = tid + r * NT;
            if (f < 3 * padded) {
                const int p = f / 3;
                nonfinite |= (f < 3 * cnt) && !pcm_finite(v[r]);
                sXYZ[f - 3 * p][p] = v[r];
            }
        }
        __syncthreads();

        const int nch = padded / C;
        for (int c = wave; c < nch; c += W) {
            const float *cx = &sXYZ[0][c * C];
            const float *cy = &sXYZ[1][c * C];
            const float *cz = &sXYZ[2][c * C];
#pragma unroll
            for (int k = 0; k < C; k += 4) {
                const pcm_f4 X4 = *reinterpret_cast<const pcm_f4 *>(cx + k);
                const pcm_f4 Y4 = *reinterpret_cast<const pcm_f4 *>(cy + k);
                const pcm_f4 Z4 = *reinterpret_cast<const pcm_f4 *>(cz + k);
                const pcm_f2 xa = X4.xy, xb = X4.zw;
                const pcm_f2 ya = Y4.xy, yb = Y4.zw;
                const pcm_f2 za = Z4.xy, zb = Z4.zw;
#pragma unroll
                for (int qq = 0; qq < QPT; ++qq) {
                    const pcm_f2 da = pcm_sqd2(xa - px[qq], ya - py[qq], za - pz[qq]);
                    const pcm_f2 db = pcm_sqd2(xb - px[qq], yb - py[qq], zb - pz[qq]);
                    // written so that hipcc forms two v_min3_f32 per 4 candidates
                    best[qq] = __builtin_fminf(__builtin_fminf(best[qq], da.x), da.y);
                    best[qq] = __builtin_fminf(__builtin_fminf(best[qq], db.x), db.y);
                }
            }
        }
    }

    // ---- merge the W waves' minima per query (the barrier is pcm_wg_or's)
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) sBest[wave][qq * 64 + lane] = best[qq];
    const int any_nonfinite = pcm_wg_or(nonfinite, sNF, W);

    // ---- one thread per query: its distance, then the record's terms.  Every
    // wave runs the reductions (uniform control flow); a thread without a
    // query contributes nothing.
    const int qi = qbase + tid;
    const bool valid = tid < QW && qi < nq;
    float d = 0.f;
    if (valid) {
        if (!any_nonfinite) {
            d = sBest[0][tid];
#pragma unroll
            for (int w = 1; w < W; ++w) d = __builtin_fminf(d, sBest[w][tid]);
        } else {
            int idx;
            pcm_ref_nn_scan(pcm_ld(Q + 3 * (size_t)qi + 0), pcm_ld(Q + 3 * (size_t)qi + 1),
                            pcm_ld(Q + 3 * (size_t)qi + 2), T, nt, d, idx);
        }
    }
    const float ws = wave_sum(d);
    if (lane == 0) sSum[wave] = ws;
#pragma unroll
    for (int t = 0; t < kEvalMaxTh; ++t) {
        const int c = __popcll(__ballot(valid && d < th.v[t]));  // strict, as loss_.py:132-133
        if (lane == 0) sCnt[wave][t] = c;
    }
    __syncthreads();
    if (tid < kEvalRec) {
        unsigned out;
        if (tid == 0) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < W; ++w) s += sSum[w];
            out = __float_as_uint(s);
        } else {
            int c = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) c += sCnt[w][tid - 1];
            out = (unsigned)c;
        }
        records[(size_t)slot * kEvalRec + tid] = out;
    }
}

// Sequential ascending sum of word `word` of records [first, first + nb):
// loads in groups of eight (independent, one latency per group), adds in order.
__device__ __forceinline__ void eval_sum_records(const unsigned *__restrict__ records, long long first, int nb,
                                                 int word, float &fs, int &ic) {
    const unsigned *rec = records + (size_t)first * kEvalRec + word;
    fs = 0.f;
    ic = 0;
    for (int k = 0; k < nb; k += 8) {
        unsigned v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (k + u < nb) ? rec[(size_t)(k + u) * kEvalRec] : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (k + u < nb) {
                fs += __uint_as_float(v[u]);
                ic += (int)v[u];
            }
        }
    }
}

// One workgroup.  Phase 1: per (cloud, direction, word) the records' sum ->
// mean_dist, counts.  Phase 2: per (cloud, threshold) the scores.  Phase 3:
// per (threshold, score) the batch mean, ascending b.  A later phase reads
// what an earlier one stored: same workgroup, same CU and L1, behind a
// workgroup barrier.
__global__ __launch_bounds__(kEvalFinT) void chamfer_eval_finalize_kernel(
    const unsigned *__restrict__ records, int b, int n, int m, int nblk1, int nblk2, int nth,
    float *__restrict__ mean_dist, int32_t *__restrict__ counts, float *__restrict__ scores,
    float *__restrict__ batch_scores) {
    const int tid = threadIdx.x;
    const long long per = (long long)nblk1 + nblk2;
    const int words = 1 + nth;
    for (long long item = tid; item < (long long)b * 2 * words; item += kEvalFinT) {
        const int word = (int)(item % words);
        const long long cd = item / words;
        const int dir = (int)(cd & 1);
        const long long cloud = cd >> 1;
        float fs;
        int ic;
        eval_sum_records(records, cloud * per + (dir ? nblk1 : 0), dir ? nblk2 : nblk1, word, fs, ic);
        if (word == 0) mean_dist[cloud * 2 + dir] = fs / (float)(dir ? m : n);
        else counts[(cloud * nth + (word - 1)) * 2 + dir] = ic;
    }
    __syncthreads();
    for (long long item = tid; item < (long long)b * nth; item += kEvalFinT) {
        const int c1 = counts[item * 2 + 0], c2 = counts[item * 2 + 1];
        const float p_x = (float)c1 / (float)n;  // share of xyz1's points within th of xyz2
        const float p_y = (float)c2 / (float)m;  // share of xyz2's points within th of xyz1
        // loss_.py:134-135: 2 p1 p2 / (p1 + p2) with p1 = p_y, NaN (0/0) -> 0
        const float f = (c1 + c2 == 0) ? 0.f : ((2.f * p_y) * p_x) / (p_y + p_x);
        scores[item * 3 + 0] = f;
        scores[item * 3 + 1] = p_x;
        scores[item * 3 + 2] = p_y;
    }
    if (!batch_scores) return;
    __syncthreads();
    if (tid < nth * 3) {
        const float *src = scores + tid;  // (t, k) = tid / 3, tid % 3
        const size_t stride = (size_t)nth * 3;
        float s = 0.f;
        for (int k = 0; k < b; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (k + u < b) ? src[(size_t)(k + u) * stride] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k + u < b) s += v[u];
        }
        batch_scores[tid] = s / (float)b;
    }
}

// 4 queries per lane once that still leaves two workgroups per compute unit
// of a whole MI355X; smaller problems take 2 for more workgroups
inline int eval_qpt(int b, int n, int m) {
    const long long blocks4 = (long long)b * ((n + 255) / 256 + (m + 255) / 256);
    return blocks4 >= 512 ? 4 : 2;
}

inline long long eval_blocks(int b, int n, int m, int &nblk1, int &nblk2) {
    const int QW = 64 * eval_qpt(b, n, m);
    nblk1 = (n + QW - 1) / QW;
    nblk2 = (m + QW - 1) / QW;
    return (long long)b * ((long long)nblk1 + nblk2);
}

template <typename TIn>
int launch_eval(const TIn *xyz1, const TIn *xyz2, int b, int n, int m, const float *thresholds, int nth,
                float *mean_dist, int32_t *counts, float *scores, float *batch_scores, void *ws, size_t ws_bytes,
                void *stream) {
    if (b < 0 || n < 0 || m < 0 || nth < 1 || nth > kEvalMaxTh) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0 || m == 0) return PCM_ERR_INVALID_ARG;
    if (!xyz1 || !xyz2 || !thresholds || !mean_dist || !counts || !scores) return PCM_ERR_INVALID_ARG;
    int nblk1, nblk2;
    const long long blocks = eval_blocks(b, n, m, nblk1, nblk2);
    if (blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < pcm_chamfer_eval_workspace_bytes(b, n, m, nth)) return PCM_ERR_WORKSPACE;
    EvalTh th;
    for (int t = 0; t < kEvalMaxTh; ++t) th.v[t] = t < nth ? thresholds[t] : -PCM_INF;
    unsigned *records = (unsigned *)ws;
    hipStream_t st = (hipStream_t)stream;
    if (eval_qpt(b, n, m) == 4)
        hipLaunchKernelGGL((chamfer_eval_scan_kernel<TIn, kEvalW, 4, kEvalChunk, kEvalTile>), dim3((unsigned)blocks),
                           dim3(64 * kEvalW), 0, st, xyz1, xyz2, n, m, nblk1, nblk2, th, records);
    else
        hipLaunchKernelGGL((chamfer_eval_scan_kernel<TIn, kEvalW, 2, kEvalChunk, kEvalTile>), dim3((unsigned)blocks),
                           dim3(64 * kEvalW), 0, st, xyz1, xyz2, n, m, nblk1, nblk2, th, records);
    hipLaunchKernelGGL(chamfer_eval_finalize_kernel, dim3(1), dim3(kEvalFinT), 0, st, records, b, n, m, nblk1, nblk2,
                       nth, mean_dist, counts, scores, batch_scores);
    return pcm_launch_status();
}

}  // namespace

extern "C" size_t pcm_chamfer_eval_workspace_bytes(int b, int n, int m, int nth) {
    if (b <= 0 || n <= 0 || m <= 0 || nth < 1 || nth > kEvalMaxTh) return 0;
    int nblk1, nblk2;
    const long long blocks = eval_blocks(b, n, m, nblk1, nblk2);
    const size_t bytes = (size_t)blocks * kEvalRec * sizeof(unsigned);
    return (bytes + 127) / 128 * 128;
}

extern "C" int pcm_chamfer_eval(const float *xyz1, const float *xyz2, int b, int n, int m, const float *thresholds,
                                int nth, float *mean_dist, int32_t *counts, float *scores, float *batch_scores,
                                void *workspace, size_t workspace_bytes, void *stream) {
    return launch_eval(xyz1, xyz2, b, n, m, thresholds, nth, mean_dist, counts, scores, batch_scores, workspace,
                       workspace_bytes, stream);
}

extern "C" int pcm_chamfer_eval_f16(const uint16_t *xyz1, const uint16_t *xyz2, int b, int n, int m,
                                    const float *thresholds, int nth, float *mean_dist, int32_t *counts,
                                    float *scores, float *batch_scores, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    return launch_eval(reinterpret_cast<const pcm_h *>(xyz1), reinterpret_cast<const pcm_h *>(xyz2), b, n, m,
                       thresholds, nth, mean_dist, counts, scores, batch_scores, workspace, workspace_bytes, stream);
}
