// chamfer_cross.hip -- the cross Chamfer matrix for MI355X (gfx950, CDNA4):
// the mean nearest-neighbour squared distance of every cloud of one set to
// every cloud of another, in both directions.  include/pcm.h has the contract;
// DESIGN.md section 3.20 has the rationale and the numbers.
//
// Scan kernel.  A workgroup of kCrossW waves owns kCrossQW consecutive query
// points of ONE cloud of the query set -- each wave 64 * kCrossQPT of them, held
// in registers for the workgroup's whole life -- and streams a run of up to
// kCrossJ consecutive clouds of the target set through LDS in SoA tiles, staged
// as chamfer_eval_scan_kernel stages them.  Every wave scans every tile against
// its own queries, two candidates at a time in packed fp32 in the pinned order
// fma(dz,dz,fma(dy,dy,dx*dx)), keeping only the running minimum (7 lane
// operations a pair): for finite input the minimum of the pinned values does
// not depend on the scan order, so it IS the dist1 / dist2 entry of
// pcm_chamfer_forward.  No wave shares a query with another, so a target
// cloud's end costs no barrier: the wave adds its minima in double (a lane its
// queries ascending, the wave by the six DPP steps), parks the sum in LDS,
// resets the minima and goes on.  The tiles are double-buffered -- the next
// tile's global loads are in flight during the scan -- so a tile costs one
// barrier.  Query loads, workgroup start-up and launch are paid once per run of
// clouds, not once per pair.
// After the run, thread jj adds target cloud jj's wave sums ascending and
// stores the mean (a query cloud of one workgroup) or one partial record.
// The opposite direction is the same kernel with the sets' roles swapped and
// the store index transposed; both directions share the launch, direction 1's
// workgroups first.  Logical workgroup ids are target-run-major, and
// pcm_xcd_remap hands an XCD a contiguous range of them, so the workgroups that
// stream the same target clouds share an L2.
//
// Finalise kernel (next on the stream, only when a query cloud spans several
// workgroups): the kernel boundary is the hand-off, as in chamfer_eval.hip --
// one thread an entry adds its records in ascending block order.
#include "pcm_common.h"

namespace {

constexpr int kCrossMaxN = PCM_CROSS_MAX_POINTS;
constexpr int kCrossW = 4;                               // waves per workgroup
constexpr int kCrossQPT = 4;                             // queries per lane
constexpr int kCrossNT = 64 * kCrossW;                   // threads per workgroup
constexpr int kCrossQW = kCrossNT * kCrossQPT;           // queries per workgroup
constexpr int kCrossTile = 1024;                         // candidates per LDS tile (3 x 4 KiB SoA, two buffers)
constexpr int kCrossChunk = 16;                          // candidates per unrolled scan step
constexpr int kCrossJ = 8;                               // target clouds per workgroup, at most
constexpr int kCrossFill = 3 * kCrossTile / kCrossNT;    // tile words per thread
constexpr int kCrossFinT = 256;                          // threads of a finalise workgroup
constexpr long long kCrossWantBlocks = 256;              // below one workgroup a compute unit the run is halved
static_assert(3 * kCrossTile % kCrossNT == 0, "every thread stages the same number of words");
static_assert((kCrossTile & (kCrossTile - 1)) == 0 && kCrossTile % kCrossChunk == 0 && kCrossChunk % 4 == 0,
              "tile: a power of two of whole chunks");
static_assert(kCrossJ <= kCrossNT, "one thread stores one target cloud's result");

struct CrossGeom {
    int nblk1, nblk2;   // workgroups per query cloud of each direction
    int run;            // target clouds per workgroup
    long long nb1, nb2; // workgroups of each direction
};

// both_dirs = false leaves direction 2 out of the grid
inline CrossGeom cross_geom(int s, int r, int n, int m, bool both_dirs) {
    CrossGeom G;
    G.nblk1 = (n + kCrossQW - 1) / kCrossQW;
    G.nblk2 = (m + kCrossQW - 1) / kCrossQW;
    G.run = kCrossJ;
    for (;;) {
        G.nb1 = (long long)s * G.nblk1 * ((r + G.run - 1) / G.run);
        G.nb2 = both_dirs ? (long long)r * G.nblk2 * ((s + G.run - 1) / G.run) : 0;
        if (G.run == 1 || G.nb1 + G.nb2 >= kCrossWantBlocks) break;
        G.run >>= 1;
    }
    return G;
}

__global__ __launch_bounds__(kCrossNT) void chamfer_cross_scan_kernel(
    const float *__restrict__ xyz1, const float *__restrict__ xyz2, int s, int r, int n, int m, int lay1, int lay2,
    int nblk1, int nblk2, int run, int nb1, float *__restrict__ mean12, float *__restrict__ mean21,
    double *__restrict__ records) {
    constexpr int W = kCrossW, QPT = kCrossQPT, TILE = kCrossTile, C = kCrossChunk, NT = kCrossNT;
    __shared__ __attribute__((aligned(16))) float sXYZ[2][3][TILE];
    __shared__ double sSum[kCrossJ][W];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // ---- which (direction, target run, query cloud, query block) this workgroup owns (uniform)
    const int slot = pcm_xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const bool first = slot < nb1;
    const int local = first ? slot : slot - nb1;
    const float *Qs = first ? xyz1 : xyz2;
    const float *Ts = first ? xyz2 : xyz1;
    const int nq = first ? n : m, nt = first ? m : n;
    const int cq = first ? s : r, ct = first ? r : s;
    const int layq = first ? lay1 : lay2, layt = first ? lay2 : lay1;
    const int nblk = first ? nblk1 : nblk2;
    const int per = cq * nblk;
    const int group = local / per;
    const int rem = local - group * per;
    const int qc = rem / nblk;
    const int blk = rem - qc * nblk;
    const int j0 = group * run;
    const int jn = min(run, ct - j0);

    // ---- this lane's query points (splatted for the packed math)
    const float *Q = Qs + (size_t)qc * nq * 3;
    const PcmLay LQ = pcm_lay(layq, nq);
    pcm_f2 px[QPT], py[QPT], pz[QPT];
    bool valid[QPT];
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
        const int qi = blk * kCrossQW + (wave * QPT + qq) * 64 + lane;
        float x = 0.f, y = 0.f, z = 0.f;
        valid[qq] = qi < nq;
        if (valid[qq]) {
            x = Q[pcm_at(LQ, qi, 0)];
            y = Q[pcm_at(LQ, qi, 1)];
            z = Q[pcm_at(LQ, qi, 2)];
        }
        px[qq] = pcm_f2{x, x};
        py[qq] = pcm_f2{y, y};
        pz[qq] = pcm_f2{z, z};
    }
    // a wave none of whose queries exist stages tiles and meets the barriers, but scans nothing
    const bool wave_scans = blk * kCrossQW + wave * QPT * 64 < nq;

    float best[QPT];
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) best[qq] = PCM_INF;

    const int tpc = (nt + TILE - 1) / TILE;  // tiles per target cloud
    const int total = jn * tpc;
    float v[kCrossFill];

    // tile `t0` of target cloud `jj` into registers: every load is issued before any LDS write; pad = +inf
    auto load_tile = [&](int jj, int t0) {
        const float *Tc = Ts + (size_t)(j0 + jj) * nt * 3;
        const int cnt = min(TILE, nt - t0);
        if (layt == 0) {
            const float *src = Tc + 3 * (size_t)t0;
#pragma unroll
            for (int k = 0; k < kCrossFill; ++k) {
                const int f = tid + k * NT;
                v[k] = (f < 3 * cnt) ? src[f] : PCM_INF;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kCrossFill; ++k) {
                const int f = tid + k * NT;
                const int c = f / TILE, p = f & (TILE - 1);
                v[k] = (p < cnt) ? Tc[(size_t)c * nt + t0 + p] : PCM_INF;
            }
        }
    };
    // the registers scattered to SoA; every word of the buffer is written
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int k = 0; k < kCrossFill; ++k) {
            const int f = tid + k * NT;
            if (layt == 0) {
                const int p = f / 3;
                sXYZ[buf][f - 3 * p][p] = v[k];
            } else {
                sXYZ[buf][f / TILE][f & (TILE - 1)] = v[k];
            }
        }
    };

    load_tile(0, 0);
    store_tile(0);
    __syncthreads();

    int jj = 0, t0 = 0;  // the tile being scanned
    for (int tt = 0; tt < total; ++tt) {
        const bool cloud_ends = t0 + TILE >= nt;
        const int njj = cloud_ends ? jj + 1 : jj;
        const int nt0 = cloud_ends ? 0 : t0 + TILE;
        const bool has_next = tt + 1 < total;
        if (has_next) load_tile(njj, nt0);

        const int buf = tt & 1;
        if (wave_scans) {
            const int cnt = min(TILE, nt - t0);
            const int nch = (cnt + C - 1) / C;
            for (int c = 0; c < nch; ++c) {
                const float *cx = &sXYZ[buf][0][c * C];
                const float *cy = &sXYZ[buf][1][c * C];
                const float *cz = &sXYZ[buf][2][c * C];
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

        if (cloud_ends) {  // uniform: the wave's sum of this target cloud, then a fresh start
            double acc = 0.0;
#pragma unroll
            for (int qq = 0; qq < QPT; ++qq) {
                if (valid[qq]) acc += (double)best[qq];
                best[qq] = PCM_INF;
            }
            const double ws = pcm_wave_sum_f64(acc);
            if (lane == 0) sSum[jj][wave] = ws;
        }

        // buffer (tt + 1) & 1 was last read in iteration tt - 1, which every wave left through its barrier
        if (has_next) store_tile((tt + 1) & 1);
        __syncthreads();
        jj = njj;
        t0 = nt0;
    }

    // ---- thread jj: target cloud jj's wave sums ascending -> the mean, or this block's record
    if (tid < jn) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < W; ++w) tot += sSum[tid][w];
        const int tc = j0 + tid;
        const size_t entry = first ? (size_t)qc * r + tc : (size_t)tc * r + qc;  // [x index, y index]
        if (nblk == 1) {
            (first ? mean12 : mean21)[entry] = (float)(tot / (double)nq);
        } else {
            double *rec = first ? records : records + (size_t)s * r * nblk1;
            rec[entry * nblk + blk] = tot;
        }
    }
}

// One thread an entry of a direction whose query clouds span several workgroups: the records ascending
__global__ __launch_bounds__(kCrossFinT) void chamfer_cross_finalize_kernel(
    const double *__restrict__ records, int s, int r, int n, int m, int nblk1, int nblk2,
    float *__restrict__ mean12, float *__restrict__ mean21) {
    const long long sr = (long long)s * r;
    const long long item = (long long)blockIdx.x * kCrossFinT + threadIdx.x;
    if (item >= 2 * sr) return;
    const bool second = item >= sr;
    const long long entry = second ? item - sr : item;
    const int nblk = second ? nblk2 : nblk1;
    float *out = second ? mean21 : mean12;
    if (nblk <= 1 || !out) return;
    const double *rec = records + (second ? (size_t)sr * nblk1 : (size_t)0) + (size_t)entry * nblk;
    double tot = 0.0;
    for (int k = 0; k < nblk; ++k) tot += rec[k];
    out[entry] = (float)(tot / (double)(second ? m : n));
}

}  // namespace

extern "C" size_t pcm_chamfer_cross_workspace_bytes(int s, int r, int n, int m) {
    if (s <= 0 || r <= 0 || n <= 0 || m <= 0) return 0;
    if ((long long)s * r > 0x7fffffffLL) return 0;  // beyond the launch limits: PCM_ERR_UNSUPPORTED
    const CrossGeom G = cross_geom(s, r, n, m, true);
    const size_t bytes = (size_t)s * r * ((size_t)G.nblk1 + G.nblk2) * sizeof(double);
    return (bytes + 127) / 128 * 128;
}

// Internal (tests): the target clouds per workgroup a call of this shape takes (kCrossJ, halved while the grid
// stays below kCrossWantBlocks workgroups); 0 for an empty problem
extern "C" int pcm_tune_chamfer_cross_run(int s, int r, int n, int m, int both_dirs) {
    if (s <= 0 || r <= 0 || n <= 0 || m <= 0) return 0;
    return cross_geom(s, r, n, m, both_dirs != 0).run;
}

extern "C" int pcm_chamfer_cross(const float *xyz1, const float *xyz2, int s, int r, int n, int m, int layout1,
                                 int layout2, float *mean12, float *mean21, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    if (s < 0 || r < 0 || n < 0 || m < 0) return PCM_ERR_INVALID_ARG;
    if ((layout1 != 0 && layout1 != 1) || (layout2 != 0 && layout2 != 1)) return PCM_ERR_INVALID_ARG;
    if (s == 0 || r == 0) return PCM_OK;
    if (n == 0 || m == 0 || !xyz1 || !xyz2 || !mean12) return PCM_ERR_INVALID_ARG;
    if (n > kCrossMaxN || m > kCrossMaxN) return PCM_ERR_UNSUPPORTED;
    const long long sr = (long long)s * r;
    if (sr > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    const CrossGeom G = cross_geom(s, r, n, m, mean21 != nullptr);
    const long long fin_blocks = (2 * sr + kCrossFinT - 1) / kCrossFinT;
    if (G.nb1 + G.nb2 > 0x7fffffffLL || fin_blocks > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < pcm_chamfer_cross_workspace_bytes(s, r, n, m)) return PCM_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return PCM_ERR_INVALID_ARG;

    double *records = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chamfer_cross_scan_kernel, dim3((unsigned)(G.nb1 + G.nb2)), dim3(kCrossNT), 0, st, xyz1, xyz2,
                       s, r, n, m, layout1, layout2, G.nblk1, G.nblk2, G.run, (int)G.nb1, mean12, mean21, records);
    if (G.nblk1 > 1 || (mean21 && G.nblk2 > 1))
        hipLaunchKernelGGL(chamfer_cross_finalize_kernel, dim3((unsigned)fin_blocks), dim3(kCrossFinT), 0, st,
                           (const double *)records, s, r, n, m, G.nblk1, G.nblk2, mean12, mean21);
    return pcm_launch_status();
}
