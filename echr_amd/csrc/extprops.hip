// Captioning external temporal-event proposals (flag_eval_what = 'SOTA_TEP'): echr_nms_segments_batch is the
// reference's eval_utils.gettopN_nms (eval_utils.py:230-256) for V videos in one launch, echr_ext_proposals_batch the selection of
// eval_utils.py:88-104 with dataloader.timestamp_to_featstamp (:292-296) and the crop of dataloader.py:515-520 behind it.
//   nms       a 1024-thread workgroup per video.  The scores go to LDS once (32 KB at the bound) and every proposal counts the proposals in
//             front of it in ascending (prop_score, index) order: its rank, the position in a stable ascending sort.  The inverse permutation
//             goes to LDS (16 KB) and thread t loads the proposals of ranks t, t + 1024, t + 2048, t + 3072 into registers -- XN_SLOTS slots of
//             (t1, t2, sent) per thread, which is where ECHR_EXTPROPS_MAX_P = 4 * 1024 comes from.  A round reads no memory but 16 LDS words
//             per reduction: every thread forms o of its alive slots against the round's best, one pass of wave shuffles reduces both the
//             cluster's pick (largest sent_score, the lowest rank among ties) and the highest rank that stays alive (the next round's best),
//             the 16 wave results cross LDS, and the owner of the next best publishes its interval.  Two barriers per round whatever P is.
//   select    a 1024-thread workgroup per video: the pick list marks an LDS flag per proposal, the proposals are walked in file order in
//             chunks of 1024 and compacted in order (wave ballots + the 16 wave totals; no atomics on the order), and each kept one is
//             converted, cropped and staged at the video's own entries; a second launch moves the lists to their batch offsets.
// o is fp64 adds, subtracts, compares and one divide in the reference's order -- no product, so nothing can be contracted: the comparison
// bits are numpy's.  The featstamp has one product, (t / duration) * T_v, rounded by round() as a finished value: contraction is switched
// off for this file so that no part of the rounding can be fused with it.  All stores are plain vector stores; the only atomic is an
// integer LDS add that forms a sum.
#include <cmath>

#include "echr_common.h"
#include "echr_internal.h"

#pragma clang fp contract(off)

namespace echr {

constexpr int XN_THREADS = 1024;
constexpr int XN_WAVES = XN_THREADS / ECHR_WAVE;
constexpr int XN_SLOTS = 4;
constexpr int XN_MAX_P = ECHR_EXTPROPS_MAX_P;
constexpr int XN_NONE = 0x7FFFFFFF;
static_assert(XN_MAX_P == XN_SLOTS * XN_THREADS, "a thread holds XN_SLOTS proposals in registers");

// the video's proposals [p0, p0 + P), or P = 0 where the offsets leave [0, P_tot] or exceed the bound (the host layer refuses both)
__device__ __forceinline__ int xn_range(const int32_t* __restrict__ prop_offset, int v, int P_tot, int& p0) {
    const int a = prop_offset[v], b = prop_offset[v + 1];
    p0 = a;
    return (a >= 0 && b >= a && b <= P_tot && b - a <= XN_MAX_P) ? b - a : 0;
}

__global__ __launch_bounds__(XN_THREADS) void nms_segments_kernel(const double* __restrict__ stamps, const double* __restrict__ prop_scores,
                                                                  const double* __restrict__ sent_score, const int32_t* __restrict__ prop_offset,
                                                                  int P_tot, double thr, int rounds, int32_t* __restrict__ pick,
                                                                  int32_t* __restrict__ count) {
    __shared__ double s_score[XN_MAX_P];
    __shared__ int s_orig[XN_MAX_P];
    __shared__ double s_cs[XN_WAVES];
    __shared__ int s_cr[XN_WAVES], s_na[XN_WAVES];
    __shared__ double s_best[2];
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & (ECHR_WAVE - 1), wave = tid / ECHR_WAVE;
    int p0;
    const int P = xn_range(prop_offset, v, P_tot, p0);          // (uniform over the workgroup)
    int32_t* __restrict__ out = pick + (long)v * rounds;
    // ---- ranks: the position of every proposal in a stable ascending sort by prop_score ----
    for (int i = tid; i < P; i += XN_THREADS) s_score[i] = prop_scores[p0 + i];
    __syncthreads();
    double mine[XN_SLOTS];
    int rank[XN_SLOTS];
#pragma unroll
    for (int c = 0; c < XN_SLOTS; ++c) {
        const int i = tid + c * XN_THREADS;
        mine[c] = i < P ? s_score[i] : 0.0;
        rank[c] = 0;
    }
    for (int j = 0; j < P; ++j) {
        const double sj = s_score[j];
#pragma unroll
        for (int c = 0; c < XN_SLOTS; ++c) {
            const int i = tid + c * XN_THREADS;
            rank[c] += (sj < mine[c] || (sj == mine[c] && j < i)) ? 1 : 0;
        }
    }
#pragma unroll
    for (int c = 0; c < XN_SLOTS; ++c) {
        const int i = tid + c * XN_THREADS;
        if (i < P) s_orig[rank[c]] = i;                  // (the ranks of i < P are a permutation of 0 .. P - 1)
    }
    __syncthreads();
    // ---- the proposals of this thread's ranks, in registers ----
    double t1[XN_SLOTS], t2[XN_SLOTS], area[XN_SLOTS], sent[XN_SLOTS];
    unsigned alive = 0u;
#pragma unroll
    for (int c = 0; c < XN_SLOTS; ++c) {
        const int r = tid + c * XN_THREADS;
        t1[c] = t2[c] = area[c] = sent[c] = 0.0;
        if (r < P) {
            const int i = p0 + s_orig[r];
            t1[c] = stamps[2 * (long)i];
            t2[c] = stamps[2 * (long)i + 1];
            area[c] = (t2[c] - t1[c]) + 1e-3;
            sent[c] = sent_score ? sent_score[i] : prop_scores[i];
            alive |= 1u << c;
        }
    }
    int best = P - 1;                                    // the alive proposal of the highest rank
    if (P > 0 && tid == ((P - 1) & (XN_THREADS - 1))) {
        const int cb = (P - 1) / XN_THREADS;
#pragma unroll
        for (int c = 0; c < XN_SLOTS; ++c)
            if (c == cb) { s_best[0] = t1[c]; s_best[1] = t2[c]; }
    }
    __syncthreads();
    int picked = 0;
    while (best >= 0 && picked < rounds) {               // (best and picked are uniform: every thread reduces the same LDS words)
        const double bt1 = s_best[0], bt2 = s_best[1];
        const double barea = (bt2 - bt1) + 1e-3;
        double cs = 0.0;
        int cr = XN_NONE, na = -1;
#pragma unroll
        for (int c = 0; c < XN_SLOTS; ++c) {
            if (!((alive >> c) & 1u)) continue;
            const int r = tid + c * XN_THREADS;
            const double tt1 = fmax(bt1, t1[c]), tt2 = fmin(bt2, t2[c]);
            const double wh = fmax(0.0, (tt2 - tt1) + 1e-3);
            const double o = wh / ((barea + area[c]) - wh);
            if (o >= thr && (cr == XN_NONE || sent[c] > cs)) { cs = sent[c]; cr = r; }          // ascending r: a tie keeps the lower rank
            if (o <= thr) na = r; else alive &= ~(1u << c);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ocs = __shfl_xor(cs, off, 64);
            const int ocr = __shfl_xor(cr, off, 64);
            const int ona = __shfl_xor(na, off, 64);
            if (ocr != XN_NONE && (cr == XN_NONE || ocs > cs || (ocs == cs && ocr < cr))) { cs = ocs; cr = ocr; }
            na = max(na, ona);
        }
        if (lane == 0) { s_cs[wave] = cs; s_cr[wave] = cr; s_na[wave] = na; }
        __syncthreads();
        cs = s_cs[0]; cr = s_cr[0]; na = s_na[0];
#pragma unroll
        for (int w = 1; w < XN_WAVES; ++w) {
            const double ocs = s_cs[w];
            const int ocr = s_cr[w];
            if (ocr != XN_NONE && (cr == XN_NONE || ocs > cs || (ocs == cs && ocr < cr))) { cs = ocs; cr = ocr; }
            na = max(na, s_na[w]);
        }
        // (the best itself has o = area / ((area + area) - area) = 1 >= thr: the cluster is never empty, and with thr < 1 the best leaves)
        if (tid == 0) out[picked] = cr != XN_NONE ? s_orig[cr] : -1;
        best = na;
        if (best >= 0 && tid == (best & (XN_THREADS - 1))) {
            const int cb = best / XN_THREADS;
#pragma unroll
            for (int c = 0; c < XN_SLOTS; ++c)
                if (c == cb) { s_best[0] = t1[c]; s_best[1] = t2[c]; }
        }
        ++picked;
        __syncthreads();                                 // s_best is written; the wave slots are read
    }
    for (int i = picked + tid; i < rounds; i += XN_THREADS) out[i] = -1;
    if (tid == 0) count[v] = picked;
}

// ---- selection, featstamps, crop ----------------------------------------------------------------------------------------------------
// dataloader.timestamp_to_featstamp's rounded coordinate, still a double: round((t / duration) * T), half away from zero
__device__ __forceinline__ double xp_row(double t, double duration, double T) {
    const double x = (t / duration) * T;
    return round(x);
}

__global__ __launch_bounds__(XN_THREADS) void ext_select_kernel(const double* __restrict__ stamps, const double* __restrict__ prop_scores,
                                                                const int32_t* __restrict__ prop_offset, const int32_t* __restrict__ rows,
                                                                const double* __restrict__ duration, const int32_t* __restrict__ pick,
                                                                const int32_t* __restrict__ pick_count, int rounds, int P_tot, int K, int topN,
                                                                double val_thres, int crop, unsigned k0, unsigned k1,
                                                                const int32_t* __restrict__ draw, int32_t* __restrict__ stage,
                                                                int32_t* __restrict__ count) {
    __shared__ int s_flag[XN_MAX_P];
    __shared__ int s_wave[XN_WAVES];
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & (ECHR_WAVE - 1), wave = tid / ECHR_WAVE;
    int p0;
    const int P = xn_range(prop_offset, v, P_tot, p0);
    const int T = rows[v];
    if (P == 0 || T < 2) {                               // (uniform) nothing to select: the reference skips such a video
        if (tid == 0) count[v] = 0;
        return;
    }
    if (pick) {
        for (int i = tid; i < P; i += XN_THREADS) s_flag[i] = 0;
        __syncthreads();
        const int n = min(max(pick_count[v], 0), rounds);
        const int32_t* __restrict__ pk = pick + (long)v * rounds;
        for (int k = tid; k < n; k += XN_THREADS) {
            const int i = pk[k];
            if (i >= 0 && i < P) s_flag[i] = 1;          // (a proposal picked twice stores the same word twice)
        }
        __syncthreads();
    }
    const double dur = duration[v], Td = (double)T;
    const unsigned stream_id = (unsigned)draw[v];
    int32_t* __restrict__ st = stage + 3 * (long)p0;
    int base = 0;                                        // kept so far (uniform)
    for (int c0 = 0; c0 < P && base < topN; c0 += XN_THREADS) {
        const int i = c0 + tid;
        const bool keep = i < P && (!pick || s_flag[i] != 0) && prop_scores[p0 + i] >= val_thres;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();                                 // the last chunk's reads of s_wave
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < XN_WAVES; ++w) {
            const int c = s_wave[w];
            wbase += w < wave ? c : 0;
            tot += c;
        }
        const int pos = base + wbase + before;
        if (keep && pos < topN) {
            const double rs = xp_row(stamps[2 * (long)(p0 + i)], dur, Td), re = xp_row(stamps[2 * (long)(p0 + i) + 1], dur, Td);
            int s = (int)fmax(fmin(rs, Td - 2.0), 0.0);                      // max(min(round(..), nfeats - 2), 0)
            int e = (int)fmin(fmax(re, (double)(s + 1)), Td - 1.0);          // min(max(round(..), start + 1), nfeats - 1)
            if (crop && e - s >= K + 1) {
                const unsigned w = philox_word((unsigned)i, stream_id, SITE_CROP, 0u, k0, k1);
                s += (int)__umulhi(w, (unsigned)(e - s - K + 1));            // uniform in [0, e - s - K]
                e = s + K;
            }
            st[3 * pos] = i;
            st[3 * pos + 1] = s;
            st[3 * pos + 2] = e;
        }
        base += tot;
    }
    if (tid == 0) count[v] = min(base, topN);
}

// Second launch, a workgroup per video: its offset is the sum of the counts in front of it; the list moves from the video's staging entries
// to that offset as index | ind = e | soi = [s, e + 1].  The last workgroup also writes the total behind both vectors.
__global__ __launch_bounds__(256) void ext_compact_kernel(const int32_t* __restrict__ prop_offset, const int32_t* __restrict__ stage, int V,
                                                          int P_tot, int cap, int32_t* __restrict__ count, int32_t* __restrict__ event_offset,
                                                          int32_t* __restrict__ index, int32_t* __restrict__ ind, int32_t* __restrict__ soi) {
    __shared__ int s_sum;
    const int v = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_sum = 0;
    __syncthreads();
    int part = 0;
    for (int u = tid; u < v; u += 256) part += count[u];
    if (part) atomicAdd(&s_sum, part);
    __syncthreads();
    const int off = s_sum, p0 = prop_offset[v];
    int n = count[v];
    if (!(p0 >= 0 && n >= 0 && (long)p0 + n <= P_tot && (long)off + n <= cap)) n = 0;          // (malformed offsets only: nothing leaves the buffers)
    const int32_t* __restrict__ st = stage + 3 * (long)p0;
    for (int i = tid; i < n; i += 256) {
        const int s = st[3 * i + 1], e = st[3 * i + 2];
        index[off + i] = st[3 * i];
        ind[off + i] = e;
        soi[2 * (off + i)] = s;
        soi[2 * (off + i) + 1] = e + 1;
    }
    if (tid == 0) {
        event_offset[v] = off;
        if (v == V - 1) { event_offset[V] = off + n; count[V] = off + n; }
    }
}

}  // namespace echr

using namespace echr;

extern "C" int echr_nms_segments_batch(const double* stamps, const double* prop_scores, const double* sent_score, const int32_t* prop_offset,
                                       int32_t V, int32_t P_tot, int32_t P_max, double nms_overlap, int32_t rounds, int32_t* pick,
                                       int32_t* count, void* stream) {
    ECHR_REQUIRE(V >= 1 && V <= ECHR_EXTPROPS_MAX_VIDEOS, "echr_nms_segments_batch: %d videos outside [1, %d]", V, ECHR_EXTPROPS_MAX_VIDEOS);
    ECHR_REQUIRE(P_tot >= 0 && P_max >= 0 && P_max <= P_tot, "echr_nms_segments_batch: P_tot = %d, P_max = %d", P_tot, P_max);
    ECHR_REQUIRE(P_max <= ECHR_EXTPROPS_MAX_P, "echr_nms_segments_batch: a video with %d proposals (at most ECHR_EXTPROPS_MAX_P = %d)", P_max, ECHR_EXTPROPS_MAX_P);
    ECHR_REQUIRE(nms_overlap >= 0.0 && nms_overlap < 1.0, "echr_nms_segments_batch: nms_overlap = %g outside [0, 1) (at 1 the best proposal never leaves the alive set)", nms_overlap);
    ECHR_REQUIRE(rounds >= 1, "echr_nms_segments_batch: rounds = %d (at least 1)", rounds);
    ECHR_REQUIRE(prop_offset && pick && count && (P_tot == 0 || (stamps && prop_scores)), "echr_nms_segments_batch: stamps, prop_scores, prop_offset, pick and count are required");
    hipLaunchKernelGGL(nms_segments_kernel, dim3(V), dim3(XN_THREADS), 0, (hipStream_t)stream, stamps, prop_scores, sent_score, prop_offset, P_tot,
                       nms_overlap, rounds, pick, count);
    return check_launch("nms_segments_batch");
}

extern "C" int echr_ext_proposals_batch(const double* stamps, const double* prop_scores, const int32_t* prop_offset, const int32_t* rows,
                                        const double* duration, const int32_t* pick, const int32_t* pick_count, int32_t rounds, int32_t V,
                                        int32_t P_tot, int32_t P_max, int32_t K, int32_t topN, double val_score_thres, int32_t crop, uint64_t seed,
                                        const int32_t* draw, int32_t* stage, int32_t cap, int32_t* count, int32_t* event_offset, int32_t* index,
                                        int32_t* ind, int32_t* soi, void* stream) {
    ECHR_REQUIRE(V >= 1 && V <= ECHR_EXTPROPS_MAX_VIDEOS, "echr_ext_proposals_batch: %d videos outside [1, %d]", V, ECHR_EXTPROPS_MAX_VIDEOS);
    ECHR_REQUIRE(P_tot >= 0 && P_max >= 0 && P_max <= P_tot, "echr_ext_proposals_batch: P_tot = %d, P_max = %d", P_tot, P_max);
    ECHR_REQUIRE(P_max <= ECHR_EXTPROPS_MAX_P, "echr_ext_proposals_batch: a video with %d proposals (at most ECHR_EXTPROPS_MAX_P = %d)", P_max, ECHR_EXTPROPS_MAX_P);
    ECHR_REQUIRE(K >= 1 && topN >= 1 && cap >= 0, "echr_ext_proposals_batch: K = %d, topN = %d, cap = %d (K and topN at least 1)", K, topN, cap);
    ECHR_REQUIRE(crop == 0 || crop == 1, "echr_ext_proposals_batch: crop = %d (0: keep over-long proposals, 1: crop them to K rows)", crop);
    ECHR_REQUIRE(!pick || (pick_count && rounds >= 1), "echr_ext_proposals_batch: a pick list needs pick_count and rounds >= 1");
    ECHR_REQUIRE(prop_offset && rows && duration && draw && count && event_offset, "echr_ext_proposals_batch: prop_offset, rows, duration, draw, count and event_offset are required");
    ECHR_REQUIRE(P_tot == 0 || (stamps && prop_scores && stage), "echr_ext_proposals_batch: stamps, prop_scores and stage are required");
    ECHR_REQUIRE(cap == 0 || (index && ind && soi), "echr_ext_proposals_batch: index, ind and soi are required");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ext_select_kernel, dim3(V), dim3(XN_THREADS), 0, st, stamps, prop_scores, prop_offset, rows, duration, pick, pick_count,
                       rounds, P_tot, K, topN, val_score_thres, crop, (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), draw, stage, count);
    hipLaunchKernelGGL(ext_compact_kernel, dim3(V), dim3(256), 0, st, prop_offset, stage, V, P_tot, cap, count, event_offset, index, ind, soi);
    return check_launch("ext_proposals_batch");
}
