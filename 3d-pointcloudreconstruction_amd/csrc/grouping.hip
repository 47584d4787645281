// grouping.hip -- ball query and the uniform loss for MI355X (gfx950, CDNA4).
// include/pcm.h has both contracts; DESIGN.md section 3.15 has the rationale
// and the numbers.  The padding rule of the ball query is pointnet2's as
// published; pointnet2_ops is not installed here, so it is NOT verified
// against that library (include/pcm.h says the same).
//
// The scan (ball_scan), shared by both entry points.  One wave owns one centre;
// the four waves of a workgroup own four centres of ONE cloud and share an LDS
// copy of it (1024-point tiles, x[], y[], z[] planes).  A wave walks the tile
// 64 points a step in index order, lane = point.  Per scale (one for
// pcm_ball_query, up to eight radii for the uniform loss, all from the same
// pass) a hit's slot is the scale's running count plus the number of hits in
// the lanes below (the ballot through v_mbcnt), so a list is the first nsample
// hits in ascending index; a scale that is full takes no further part and a
// wave whose scales are all full stops reading.  The workgroup stops staging
// tiles once no wave needs one (pcm_wg_or: one barrier).
//
// pcm_uniform_loss.  Four launches, all deterministic:
//   1. pcm_fps (csrc/sampling.hip, through its exported host function) writes
//      the seeds and their coordinates into the workspace;
//   2. uniform_group_kernel: the scan around every seed with the lists AND the
//      members' coordinates kept in LDS; then every lane owns one slot, the
//      scales side by side (40 slots at the default sizes; 64 a pass), scans
//      its group for the two smallest (distance, slot) pairs, the wave adds
//      each scale's u values in double by DPP, lane q finishes scale q, and
//      every slot writes one record (i, j, g[3]) -- its contribution to point
//      i, the negative to point j; (-1, -1, 0) when it has none -- and the wave
//      one double, its weighted terms;
//   3. uniform_gather_kernel: one lane per point sums the records of its cloud
//      that name it, in record order (four waves, a quarter of every tile each,
//      the four partial sums added in ascending order): no float atomics;
//   4. uniform_finish_kernel: one workgroup adds the seeds' doubles in a fixed order.
#include "pcm_common.h"

namespace {

constexpr int kBallMaxNsample = PCM_BALL_MAX_NSAMPLE;
constexpr int kBallMaxN = PCM_KNN_MAX_POINTS;
constexpr int kBallTile = 1024;   // cloud points per LDS tile (12 KiB)
constexpr int kBallWaves = 4;     // centres (waves) per workgroup
constexpr int kBallThreads = 64 * kBallWaves;

constexpr int kUniMaxScales = PCM_UNIFORM_MAX_SCALES;
constexpr int kUniMaxSlots = kUniMaxScales * kBallMaxNsample;  // slots of one seed, all scales (48 KiB of lists a workgroup)
constexpr int kUniPoints = 64;    // points per workgroup of the gather kernel: one per lane
constexpr int kUniWaves = 4;      // waves that share them: each scans a quarter of every tile's records
constexpr int kUniThreads = kUniPoints * kUniWaves;
constexpr int kUniTile = 1024;    // records per tile: a quarter to a wave, four to a lane
constexpr int kFinishThreads = 1024;  // threads of the kernel that adds the seeds' doubles

// the scales of one call, as a kernel argument: squared radius, list length and
// the list's first slot among a centre's slots
template <int Q>
struct BallScales {
    float r2[Q];
    int ns[Q];
    int off[Q];
};

struct UniformArgs {
    BallScales<kUniMaxScales> sc;
    double weight[kUniMaxScales];
    double coef[kUniMaxScales];  // weight * 2 / ((L + 1e-8) b npoint nsample)
    double expect_len;           // L
    double len_eps;              // L + 1e-8
    int nscales;
    int total;                   // slots of one seed: the sum of ns
    int max_ns;                  // the longest group
};

__device__ __forceinline__ int ball_prefix(unsigned long long bal) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
}

// The scan of one workgroup: wave `wave` around (cx, cy, cz) when `active`.
// cnt[q] = min(hits, ns[q]) and first[q] = the lowest hit (0 without one), both
// wave-uniform; store(q, slot, k, x, y, z) is called by the lane that holds hit
// number `slot` < ns[q] of scale q: point k of the cloud.  A NaN distance fails
// '<' and a lane past the cloud is masked: every k is in [0, n).  Full
// workgroup, uniform control flow; sX/sY/sZ: kBallTile floats each, flags:
// kBallWaves ints.
template <int Q, typename Store>
__device__ __forceinline__ void ball_scan(const float *__restrict__ P, PcmLay L, int n, const BallScales<Q> &sc,
                                          int nscales, bool active, float cx, float cy, float cz, float *sX,
                                          float *sY, float *sZ, int *flags, int (&cnt)[Q], int (&first)[Q],
                                          Store store) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        cnt[q] = 0;
        first[q] = 0;
    }
    for (int t0 = 0; t0 < n; t0 += kBallTile) {
        if (t0 > 0) __syncthreads();  // the previous tile has been read, and the votes of its round
        const int cntT = min(kBallTile, n - t0);
#pragma unroll 4
        for (int p = tid; p < cntT; p += kBallThreads) {  // a full tile is four points a thread
            sX[p] = P[pcm_at(L, t0 + p, 0)];
            sY[p] = P[pcm_at(L, t0 + p, 1)];
            sZ[p] = P[pcm_at(L, t0 + p, 2)];
        }
        bool need = false;
#pragma unroll
        for (int q = 0; q < Q; ++q) need |= q < nscales && cnt[q] < sc.ns[q];
        need &= active;
        if (!pcm_wg_or(need, flags, kBallWaves)) break;  // its barrier also publishes the tile
        if (!need) continue;
        for (int c0 = 0; c0 < cntT; c0 += 64) {
            const int p = c0 + lane;
            const bool in = p < cntT;
            const float x = sX[in ? p : 0], y = sY[in ? p : 0], z = sZ[in ? p : 0];
            const float d = pcm_sqd(x - cx, y - cy, z - cz);
            bool more = false;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (q < nscales && cnt[q] < sc.ns[q]) {
                    const bool hit = in && d < sc.r2[q];
                    const unsigned long long bal = __ballot(hit);
                    if (bal != 0ull) {
                        const int slot = cnt[q] + ball_prefix(bal);
                        if (hit && slot < sc.ns[q]) store(q, slot, t0 + p, x, y, z);
                        if (cnt[q] == 0) first[q] = t0 + c0 + __builtin_ctzll(bal);
                        cnt[q] = min(sc.ns[q], cnt[q] + __builtin_popcountll(bal));
                    }
                    more |= cnt[q] < sc.ns[q];
                }
            }
            if (!more) break;
        }
    }
}

// centres blk * 4 + wave of cloud blockIdx.x / nblk against the cloud's n points
__global__ __launch_bounds__(kBallThreads) void ball_query_kernel(const float *__restrict__ xyz,
                                                                  const float *__restrict__ new_xyz, int n, int s,
                                                                  int planes_x, int planes_c, BallScales<1> sc,
                                                                  int nblk, int *__restrict__ idx_out,
                                                                  int *__restrict__ cnt_out) {
    __shared__ float sX[kBallTile], sY[kBallTile], sZ[kBallTile];
    __shared__ int flags[kBallWaves];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = blockIdx.x / nblk;
    const int c = (blockIdx.x - bi * nblk) * kBallWaves + wave;
    const bool active = c < s;
    const PcmLay Lx = pcm_lay(planes_x, n), Lc = pcm_lay(planes_c, s);
    const float *P = xyz + (size_t)bi * n * 3;
    const float *C = new_xyz + (size_t)bi * s * 3;
    const float cx = active ? C[pcm_at(Lc, c, 0)] : 0.f;
    const float cy = active ? C[pcm_at(Lc, c, 1)] : 0.f;
    const float cz = active ? C[pcm_at(Lc, c, 2)] : 0.f;
    const int nsample = sc.ns[0];
    int *out = idx_out + ((size_t)bi * s + (active ? c : 0)) * nsample;

    int cnt[1], first[1];
    ball_scan<1>(P, Lx, n, sc, 1, active, cx, cy, cz, sX, sY, sZ, flags, cnt, first,
                 [&](int, int slot, int k, float, float, float) { out[slot] = k; });
    if (!active) return;
    // pointnet2's padding: the first hit repeated; no hit at all leaves its zero-initialised output
    for (int t = cnt[0] + lane; t < nsample; t += 64) out[t] = first[0];
    if (cnt_out && lane == 0) cnt_out[(size_t)bi * s + c] = cnt[0];
}

// the scale that slot sl of a seed belongs to (the last one that begins at or before it), the scale's
// first slot and its length
__device__ __forceinline__ void uni_scale_of(const UniformArgs &a, int sl, int &q, int &at0, int &ns) {
    q = 0;
    at0 = 0;
    ns = a.sc.ns[0];
#pragma unroll
    for (int k = 1; k < kUniMaxScales; ++k) {
        if (k < a.nscales && sl >= a.sc.off[k]) {
            q = k;
            at0 = a.sc.off[k];
            ns = a.sc.ns[k];
        }
    }
}

__device__ __forceinline__ double uni_readlane_f64(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane),
                            __builtin_amdgcn_readlane(__double2loint(x), lane));
}

// seeds blk * 4 + wave of cloud blockIdx.x / nblk: their groups at every scale,
// the records of every slot and the seed's weighted terms
__global__ __launch_bounds__(kBallThreads) void uniform_group_kernel(const float *__restrict__ xyz, int n, int planes,
                                                                     int npoint, int nblk, UniformArgs a,
                                                                     const float *__restrict__ centres,
                                                                     double *__restrict__ partial,
                                                                     int2 *__restrict__ rec_ij,
                                                                     float *__restrict__ rec_g, size_t rec_stride,
                                                                     int *__restrict__ groups_out, int want_grad) {
    __shared__ float sX[kBallTile], sY[kBallTile], sZ[kBallTile];
    __shared__ int flags[kBallWaves];
    // a wave's lists: idx, x, y, z, e and v* of a.total slots each (dynamic: 3.75 KiB a workgroup at the
    // default scales, 48 KiB at eight scales of 64)
    extern __shared__ __attribute__((aligned(16))) int sLists[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = blockIdx.x / nblk;
    const int s = (blockIdx.x - bi * nblk) * kBallWaves + wave;
    const bool active = s < npoint;
    const PcmLay L = pcm_lay(planes, n);
    const float *P = xyz + (size_t)bi * n * 3;
    // the seed's coordinates as pcm_fps wrote them beside its index (p[seed] bit for bit): no dependent read
    const float *C = centres + ((size_t)bi * npoint + (active ? s : 0)) * 3;
    const float cx = C[0], cy = C[1], cz = C[2];
    int *gi = sLists + wave * 6 * a.total;
    float *gx = (float *)(gi + a.total), *gy = gx + a.total, *gz = gy + a.total;

    int cnt[kUniMaxScales], first[kUniMaxScales];
    ball_scan<kUniMaxScales>(P, L, n, a.sc, a.nscales, active, cx, cy, cz, sX, sY, sZ, flags, cnt, first,
                             [&](int q, int slot, int k, float x, float y, float z) {
                                 const int at = a.sc.off[q] + slot;
                                 gi[at] = k;
                                 gx[at] = x;
                                 gy[at] = y;
                                 gz[at] = z;
                             });
    __syncthreads();  // the hits' slots are in LDS
    // padding: the first hit and its coordinates (slot 0 of the list); point 0 without a hit
#pragma unroll
    for (int q = 0; q < kUniMaxScales; ++q) {
        if (q < a.nscales && active && cnt[q] < a.sc.ns[q]) {
            const int at0 = a.sc.off[q];
            const bool none = cnt[q] == 0;
            const float fx = none ? P[pcm_at(L, 0, 0)] : gx[at0];
            const float fy = none ? P[pcm_at(L, 0, 1)] : gy[at0];
            const float fz = none ? P[pcm_at(L, 0, 2)] : gz[at0];
            for (int t = cnt[q] + lane; t < a.sc.ns[q]; t += 64) {
                gi[at0 + t] = first[q];
                gx[at0 + t] = fx;
                gy[at0 + t] = fy;
                gz[at0 + t] = fz;
            }
        }
    }
    __syncthreads();  // the lists are complete
    if (!active) return;

    const size_t row = (size_t)bi * npoint + s;
    if (groups_out) {
        for (int t = lane; t < a.total; t += 64) groups_out[row * a.total + t] = gi[t];
    }
    // Every lane owns one slot of the seed, all scales side by side (40 slots at the default sizes), 64
    // slots a pass.  Pass 1: the slot's nearest other member, its u, and the scales' sums of u.
    float *sD = gz + a.total;          // e_t of every slot
    int *sV = (int *)(sD + a.total);   // and v*
    double mysum = 0.0;  // lane q: the sum of scale q's u values
    for (int c0 = 0; c0 < a.total; c0 += 64) {
        const int sl = c0 + lane;
        const bool own = sl < a.total;
        int myq, at0, ns;
        uni_scale_of(a, sl, myq, at0, ns);
        const int me = own ? sl : 0;
        const float px = gx[me], py = gy[me], pz = gz[me];
        // the two smallest (d, v) in ascending v: the strict '<' keeps the lower slot on equal d, and
        // NaN and +inf fail it against the +inf of an empty place (pcm_knn's rules at k = 2)
        float d0 = PCM_INF, d1 = PCM_INF;
        int v0 = -1, v1 = -1;
#pragma unroll 4
        for (int v = 0; v < a.max_ns; ++v) {  // to the longest group: a lane past its own takes nothing
            const bool on = v < ns;
            const int at = at0 + (on ? v : 0);
            const float d = pcm_sqd(gx[at] - px, gy[at] - py, gz[at] - pz);
            const bool lo = on & (d < d0), mid = on & (d < d1);
            d1 = lo ? d0 : (mid ? d : d1);
            v1 = lo ? v0 : (mid ? v : v1);
            d0 = lo ? d : d0;
            v0 = lo ? v : v0;
        }
        if (own) {
            sD[me] = d1;
            sV[me] = v1;
        }
        const float u = __builtin_sqrtf(d1) + 1e-8f;  // the root correctly rounded
        for (int q = 0; q < a.nscales; ++q) {
            if (a.sc.off[q] >= c0 + 64 || a.sc.off[q] + a.sc.ns[q] <= c0) continue;  // no slot of q in this pass
            const double part = pcm_wave_sum_f64(own && myq == q ? (double)u : 0.0);
            if (lane == q) mysum += part;
        }
    }
    // lane q finishes scale q: m, the weighted term and the gradient's coefficient
    double w = 0.0, coef = 0.0;
    int nsq = 1;
#pragma unroll
    for (int q = 0; q < kUniMaxScales; ++q) {
        if (lane == q) {
            w = a.weight[q];
            coef = a.coef[q];
            nsq = a.sc.ns[q];
        }
    }
    const double dm = mysum / (double)nsq - a.expect_len;
    const double wt = w * (dm * dm / a.len_eps);
    const double cdm = coef * dm;
    double wterm = 0.0;  // over the scales, ascending
    for (int q = 0; q < a.nscales; ++q) wterm += uni_readlane_f64(wt, q);
    if (lane == 0) partial[row] = wterm;
    if (!want_grad) return;

    // Pass 2: one record a slot
    const size_t rec0 = row * a.total;
    for (int c0 = 0; c0 < a.total; c0 += 64) {
        const int sl = c0 + lane;
        int myq, at0, ns;
        uni_scale_of(a, sl, myq, at0, ns);
        float cf = 0.f;
        for (int q = 0; q < a.nscales; ++q) {
            const float cq = (float)uni_readlane_f64(cdm, q);
            cf = myq == q ? cq : cf;
        }
        if (sl < a.total) {
            const float d1 = sD[sl];
            const bool live = d1 > 0.f && d1 < PCM_INF;  // a zero distance adds nothing: the subgradient
            const int nb = at0 + (live ? sV[sl] : 0);
            const float root = __builtin_sqrtf(d1);
            rec_ij[rec0 + sl] = live ? int2{gi[sl], gi[nb]} : int2{-1, -1};
            rec_g[rec0 + sl] = live ? cf * ((gx[sl] - gx[nb]) / root) : 0.f;
            rec_g[rec_stride + rec0 + sl] = live ? cf * ((gy[sl] - gy[nb]) / root) : 0.f;
            rec_g[2 * rec_stride + rec0 + sl] = live ? cf * ((gz[sl] - gz[nb]) / root) : 0.f;
        }
    }
}

// points blk * 64 + lane of cloud blockIdx.x / nblk: the sum of the cloud's nrec
// records that name them.  Records are taken in tiles of 1024; wave w holds the
// w-th quarter of a tile in registers, lane = record (four steps of 64, every
// load of the tile issued before the first use).  A record matters to the
// workgroup only if its i or j is one of the 64 points -- about one record in
// ten at the default sizes -- so the wave ballots that test and walks the set
// bits in ascending order: the record's (i, j, g) come to every lane through
// v_readlane and the one or two lanes it names add it.  Wave 0 adds the four
// partial sums.
__global__ __launch_bounds__(kUniThreads) void uniform_gather_kernel(int n, int planes, int nblk, int nrec,
                                                                     const int2 *__restrict__ rec_ij,
                                                                     const float *__restrict__ rec_g,
                                                                     size_t rec_stride, float *__restrict__ gradxyz) {
    constexpr int kQuarter = kUniTile / kUniWaves;
    constexpr int kSteps = kQuarter / 64;
    __shared__ float sAcc[3][kUniWaves - 1][kUniPoints];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = blockIdx.x / nblk;
    const int i0 = (blockIdx.x - bi * nblk) * kUniPoints;
    const int i = i0 + lane;
    const int2 *E = rec_ij + (size_t)bi * nrec;
    const float *G = rec_g + (size_t)bi * nrec;

    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int r0 = wave * kQuarter; r0 < nrec; r0 += kUniTile) {
        int2 e[kSteps];
        float gx[kSteps], gy[kSteps], gz[kSteps];
#pragma unroll
        for (int u = 0; u < kSteps; ++u) {
            const int r = r0 + u * 64 + lane;
            const bool in = r < nrec;  // a record past the end names nobody
            const size_t at = in ? r : 0;
            e[u] = in ? E[at] : int2{-1, -1};
            gx[u] = G[at];
            gy[u] = G[rec_stride + at];
            gz[u] = G[2 * rec_stride + at];
        }
#pragma unroll
        for (int u = 0; u < kSteps; ++u) {
            // -1 (no contribution) wraps far above 64
            const bool mine = (unsigned)(e[u].x - i0) < (unsigned)kUniPoints ||
                              (unsigned)(e[u].y - i0) < (unsigned)kUniPoints;
            unsigned long long todo = __ballot(mine);
            while (todo != 0ull) {  // ascending record order; as point i before as point j
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int ri = __builtin_amdgcn_readlane(e[u].x, l), rj = __builtin_amdgcn_readlane(e[u].y, l);
                const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gx[u]), l));
                const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gy[u]), l));
                const float z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gz[u]), l));
                if (ri == i) {
                    ax += x;
                    ay += y;
                    az += z;
                }
                if (rj == i) {
                    ax -= x;
                    ay -= y;
                    az -= z;
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
    if (wave == 0 && i < n) {
#pragma unroll
        for (int w = 0; w < kUniWaves - 1; ++w) {
            ax += sAcc[0][w][lane];
            ay += sAcc[1][w][lane];
            az += sAcc[2][w][lane];
        }
        const PcmLay L = pcm_lay(planes, n);
        float *O = gradxyz + (size_t)bi * n * 3;
        O[pcm_at(L, i, 0)] = ax;
        O[pcm_at(L, i, 1)] = ay;
        O[pcm_at(L, i, 2)] = az;
    }
}

// loss_out[0] = (sum of the seeds' doubles) * inv_count in a fixed order: thread t adds entries t,
// t + 1024, .. ascending, every wave its 64 threads by the six DPP steps, thread 0 the sixteen waves' sums
// ascending
__global__ __launch_bounds__(kFinishThreads) void uniform_finish_kernel(const double *__restrict__ partial,
                                                                        int count, double inv_count,
                                                                        float *__restrict__ loss_out) {
    __shared__ double sWave[kFinishThreads / 64];
    double acc = 0.0;
    for (int p = threadIdx.x; p < count; p += kFinishThreads) acc += partial[p];
    const double wsum = pcm_wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) sWave[threadIdx.x >> 6] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < kFinishThreads / 64; ++w) total += sWave[w];
        loss_out[0] = (float)(total * inv_count);
    }
}

inline int ball_blocks(int s) { return (s + kBallWaves - 1) / kBallWaves; }
inline int uni_blocks(int n) { return (n + kUniPoints - 1) / kUniPoints; }

// the layout of the uniform loss's workspace: the seeds (int64), the seeds' doubles, the records'
// (i, j) pairs and their g planes, the seeds' coordinates
inline size_t uni_rows(int b, int npoint) { return (size_t)b * npoint; }
inline size_t uni_bytes(int b, int npoint, int total) {
    return uni_rows(b, npoint) * (sizeof(int64_t) + sizeof(double) + 3 * sizeof(float)) +
           uni_rows(b, npoint) * total * (sizeof(int2) + 3 * sizeof(float));
}

// the checks the workspace size shares with the call: 0 = fine
int uni_check_scales(int nscales, const int *nsample) {
    if (nscales < 1 || nscales > kUniMaxScales || !nsample) return PCM_ERR_INVALID_ARG;
    for (int q = 0; q < nscales; ++q)
        if (nsample[q] < 2) return PCM_ERR_INVALID_ARG;
    return PCM_OK;
}

}  // namespace

extern "C" int pcm_ball_query(const float *xyz, const float *new_xyz, int b, int n, int s, int layout_xyz,
                              int layout_new, float radius, int nsample, int32_t *idx_out, int32_t *cnt_out,
                              void *stream) {
    if (b < 0 || n < 0 || s < 0 || nsample < 1) return PCM_ERR_INVALID_ARG;
    if ((layout_xyz != 0 && layout_xyz != 1) || (layout_new != 0 && layout_new != 1)) return PCM_ERR_INVALID_ARG;
    if (!__builtin_isfinite(radius) || !(radius > 0.f)) return PCM_ERR_INVALID_ARG;
    if (b == 0) return PCM_OK;
    if (n == 0 || s == 0 || !xyz || !new_xyz || !idx_out) return PCM_ERR_INVALID_ARG;
    if (nsample > kBallMaxNsample || n > kBallMaxN) return PCM_ERR_UNSUPPORTED;
    const int nblk = ball_blocks(s);
    if ((long long)b * nblk > 0x7fffffffLL) return PCM_ERR_UNSUPPORTED;  // the grid
    BallScales<1> sc;
    sc.r2[0] = radius * radius;
    sc.ns[0] = nsample;
    sc.off[0] = 0;
    hipLaunchKernelGGL(ball_query_kernel, dim3((unsigned)((long long)b * nblk)), dim3(kBallThreads), 0,
                       (hipStream_t)stream, xyz, new_xyz, n, s, layout_xyz, layout_new, sc, nblk, (int *)idx_out,
                       (int *)cnt_out);
    return pcm_launch_status();
}

extern "C" size_t pcm_uniform_workspace_bytes(int b, int n, int npoint, int nscales, const int *nsample) {
    if (b <= 0 || n <= 0 || npoint <= 0 || uni_check_scales(nscales, nsample) != PCM_OK) return 0;
    long long total = 0;
    for (int q = 0; q < nscales; ++q) total += nsample[q];
    if (total > 0x7fffffffLL) return 0;
    return uni_bytes(b, npoint, (int)total);
}

extern "C" int pcm_uniform_loss(const float *xyz, int b, int n, int layout, int npoint, int nscales,
                                const int *nsample, const float *ball_radius, const double *weight,
                                double expect_len, float *loss_out, float *gradxyz, int32_t *groups_out,
                                void *workspace, size_t ws_bytes, void *stream) {
    if (b < 0 || n < 0 || (layout != 0 && layout != 1)) return PCM_ERR_INVALID_ARG;
    if (npoint < 1 || !ball_radius || !weight || uni_check_scales(nscales, nsample) != PCM_OK)
        return PCM_ERR_INVALID_ARG;
    if (!__builtin_isfinite(expect_len) || !(expect_len > 0.0)) return PCM_ERR_INVALID_ARG;
    for (int q = 0; q < nscales; ++q) {
        if (!__builtin_isfinite(ball_radius[q]) || !(ball_radius[q] > 0.f) || !__builtin_isfinite(weight[q]))
            return PCM_ERR_INVALID_ARG;
    }
    if (b == 0) return PCM_OK;
    if (n == 0 || !xyz || !loss_out) return PCM_ERR_INVALID_ARG;
    for (int q = 0; q < nscales; ++q)
        if (nsample[q] > kBallMaxNsample) return PCM_ERR_UNSUPPORTED;
    if (n > kBallMaxN) return PCM_ERR_UNSUPPORTED;
    const int gblk = ball_blocks(npoint), pblk = uni_blocks(n);
    if ((long long)b * gblk > 0x7fffffffLL || (long long)b * pblk > 0x7fffffffLL ||
        (long long)b * npoint > 0x7fffffffLL || (long long)npoint * kUniMaxSlots > 0x7fffffffLL)
        return PCM_ERR_UNSUPPORTED;  // the grids, and a cloud's record count
    if (!workspace || ws_bytes < pcm_uniform_workspace_bytes(b, n, npoint, nscales, nsample))
        return PCM_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return PCM_ERR_INVALID_ARG;

    UniformArgs a = {};
    a.nscales = nscales;
    a.expect_len = expect_len;
    a.len_eps = expect_len + 1e-8;
    for (int q = 0; q < nscales; ++q) {
        a.sc.r2[q] = ball_radius[q] * ball_radius[q];
        a.sc.ns[q] = nsample[q];
        a.sc.off[q] = a.total;
        a.total += nsample[q];
        a.max_ns = nsample[q] > a.max_ns ? nsample[q] : a.max_ns;
        a.weight[q] = weight[q];
        a.coef[q] = weight[q] * 2.0 / (a.len_eps * (double)b * (double)npoint * (double)nsample[q]);
    }
    const size_t rows = uni_rows(b, npoint), rec_stride = rows * a.total;
    int64_t *seeds = (int64_t *)workspace;
    double *partial = (double *)(seeds + rows);
    int2 *rec_ij = (int2 *)(partial + rows);
    float *rec_g = (float *)(rec_ij + rec_stride);
    float *centres = rec_g + 3 * rec_stride;

    const int st = pcm_fps(xyz, b, n, layout, npoint, 0, seeds, centres, stream);
    if (st != PCM_OK) return st;
    hipLaunchKernelGGL(uniform_group_kernel, dim3((unsigned)(b * gblk)), dim3(kBallThreads),
                       (size_t)kBallWaves * 6 * a.total * sizeof(int), (hipStream_t)stream,
                       xyz, n, layout, npoint, gblk, a, (const float *)centres, partial, rec_ij, rec_g, rec_stride,
                       (int *)groups_out, gradxyz ? 1 : 0);
    if (gradxyz) {
        hipLaunchKernelGGL(uniform_gather_kernel, dim3((unsigned)(b * pblk)), dim3(kUniThreads), 0,
                           (hipStream_t)stream, n, layout, pblk, npoint * a.total, (const int2 *)rec_ij,
                           (const float *)rec_g, rec_stride, gradxyz);
    }
    hipLaunchKernelGGL(uniform_finish_kernel, dim3(1), dim3(kFinishThreads), 0, (hipStream_t)stream,
                       (const double *)partial, (int)rows, 1.0 / ((double)b * (double)npoint), loss_out);
    return pcm_launch_status();
}
