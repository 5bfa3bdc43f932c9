// Proposal targets and caption-event samples from ground-truth segments (echr_tap_targets_batch / echr_prop_events_batch, DESIGN.md
// section 4x): the supervision that dataloader.get_vid_data / get_data / get_shuffle_list build per video on the host.
//   targets   a workgroup per tile of TT_ROWS concatenated rows, threads along k: the owning video's segments staged once in LDS (widened
//             by 0.01 on both sides), the fp64 IoU of anchor [t-k-1, t] against each in order, five coalesced stores per cell, the count
//             of good cells by one integer atomic add per (workgroup, video)
//   events    a 1024-thread workgroup per video over its good cells.  'all': ordered compaction in row-major order (wave ballots + a scan
//             of the 16 wave totals; no atomics on the order).  'sampled': every good cell p = t*K + k draws a Philox word; an exact 4-pass
//             radix select finds the word of rank min(n_good, cap), the survivors (all smaller words, ties by position) go to LDS as
//             (word, p) keys, a bitonic sort orders them, and the list is written in ascending (word, p) order
// The IoU is fp64 adds, subtracts, compares and one divide in the reference's order -- no product, so nothing can be contracted: its bits
// are the host's.  All stores are plain vector stores; integer atomics only (order-free).
#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

constexpr int TT_THREADS = 256;
constexpr int TT_ROWS = 8;
constexpr int TT_MAX_GT = ECHR_TARGETS_MAX_GT;
constexpr int PE_THREADS = 1024;
constexpr int PE_WAVES = PE_THREADS / ECHR_WAVE;
constexpr int PE_MAX_CAP = ECHR_PROP_MAX_SAMPLE;
static_assert(PE_MAX_CAP == PE_THREADS, "the survivors' sort holds one key per thread");

// the video that owns concatenated row i: the first v with off[v + 1] > i
__device__ __forceinline__ int tt_video_of(const int32_t* __restrict__ off, int V, int i) {
    int lo = 0, hi = V;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    return min(lo, V - 1);
}

__global__ __launch_bounds__(TT_THREADS) void tt_zero_kernel(int32_t* __restrict__ p, int n) {
    const int i = blockIdx.x * TT_THREADS + threadIdx.x;
    if (i < n) p[i] = 0;
}

__global__ __launch_bounds__(TT_THREADS) void tap_targets_kernel(const int32_t* __restrict__ row_offset, const int32_t* __restrict__ gt_offset,
                                                                 const int32_t* __restrict__ gt, int V, int T_tot, int G_tot, int K, float thr,
                                                                 float thr_good, float* __restrict__ iou, int32_t* __restrict__ gts_index,
                                                                 float* __restrict__ tap_masks, float* __restrict__ tap_labels,
                                                                 int32_t* __restrict__ good_gt, int32_t* __restrict__ n_good) {
    __shared__ double s_seg[TT_MAX_GT][2];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * TT_ROWS, row1 = min(row0 + TT_ROWS, T_tot);
    int staged = -1, G = 0, cnt = 0;
    if (tid == 0) s_cnt = 0;
    for (int row = row0; row < row1; ++row) {          // (everything that steers the barriers is uniform over the workgroup)
        const int v = tt_video_of(row_offset, V, row);
        if (v != staged) {
            __syncthreads();                             // the last video's reads of s_seg, and s_cnt = 0
            if (staged >= 0) {
                if (cnt) atomicAdd(&s_cnt, cnt);
                __syncthreads();
                if (tid == 0) { if (s_cnt) atomicAdd(&n_good[staged], s_cnt); s_cnt = 0; }
                cnt = 0;
            }
            // offsets outside [0, G_tot] or more than TT_MAX_GT segments (the host layer refuses both): the part that fits
            const int g0 = min(max(gt_offset[v], 0), G_tot), g1 = min(max(gt_offset[v + 1], g0), G_tot);
            G = min(g1 - g0, TT_MAX_GT);
            for (int i = tid; i < G; i += TT_THREADS) {
                s_seg[i][0] = (double)gt[2 * (g0 + i)] - 0.01;
                s_seg[i][1] = (double)gt[2 * (g0 + i) + 1] + 0.01;
            }
            staged = v;
            __syncthreads();
        }
        const int t = row - row_offset[v];
        const double end_i = (double)t;
        const long base = (long)row * K;
        for (int k = tid; k < K; k += TT_THREADS) {
            const bool valid = t >= k + 1;
            double best = 0.0;
            int index = 0;
            if (valid) {
                const double start_i = (double)(t - k - 1);
                index = -1;
                for (int i = 0; i < G; ++i) {
                    const double s = s_seg[i][0], e = s_seg[i][1];
                    const double inter = fmax(0.0, fmin(e, end_i) - fmax(s, start_i));
                    const double uni = fmin(fmax(e, end_i) - fmin(s, start_i), ((e - s) + end_i) - start_i);
                    const double ov = inter / (uni + 1e-8);
                    if (ov >= best) { best = ov; index = i; }
                }
            }
            const float f = (float)best;
            const bool good = valid && f >= thr_good && index >= 0;
            iou[base + k] = f;
            gts_index[base + k] = index;
            tap_masks[base + k] = valid ? 1.f : 0.f;
            tap_labels[base + k] = f >= thr ? 1.f : 0.f;
            good_gt[base + k] = good ? index : -1;
            cnt += good ? 1 : 0;
        }
    }
    __syncthreads();
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0 && staged >= 0 && s_cnt) atomicAdd(&n_good[staged], s_cnt);
}

// ---- event lists ------------------------------------------------------------------------------------------------------------------
// Exclusive rank of this thread's flag among the workgroup's flags in thread order, and the workgroup's total (to every thread).
// Two barriers; s_wave holds PE_WAVES ints.
__device__ __forceinline__ int pe_rank(int flag, int* __restrict__ s_wave, int& total) {
    const int lane = threadIdx.x & (ECHR_WAVE - 1), wave = threadIdx.x / ECHR_WAVE;
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                     // the previous call's reads of s_wave
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < PE_WAVES; ++w) {
        const int c = s_wave[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    total = tot;
    return base + before;
}

__device__ __forceinline__ void pe_write(int32_t* __restrict__ ev, int i, int p, int K, int gt) {
    ev[3 * i] = p / K;
    ev[3 * i + 1] = p % K;
    ev[3 * i + 2] = gt;
}

__global__ __launch_bounds__(PE_THREADS) void prop_events_kernel(const int32_t* __restrict__ good_gt, const int32_t* __restrict__ row_offset,
                                                                 int T_tot, int K, int cap, int sampled, unsigned k0, unsigned k1,
                                                                 const int32_t* __restrict__ draw, int32_t* __restrict__ events,
                                                                 int32_t* __restrict__ n_events) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_rank;
    __shared__ int s_wave[PE_WAVES];
    __shared__ int s_base, s_eq;
    __shared__ unsigned long long s_key[PE_THREADS];
    const int v = blockIdx.x, tid = threadIdx.x;
    const int r0 = row_offset[v], r1 = row_offset[v + 1];
    int32_t* __restrict__ ev = events + (long)v * cap * 3;
    if (!(r0 >= 0 && r1 > r0 && r1 <= T_tot)) {          // (uniform) offsets outside [0, T_tot]: no events
        for (int i = tid; i < 3 * cap; i += PE_THREADS) ev[i] = -1;
        if (tid == 0) n_events[v] = 0;
        return;
    }
    const int32_t* __restrict__ g = good_gt + (long)r0 * K;
    const int n = (r1 - r0) * K;                         // (T_tot * K < 2^31: checked by the entry)
    if (tid == 0) { s_base = 0; s_eq = 0; }
    __syncthreads();
    if (!sampled) {
        for (int c0 = 0; c0 < n; c0 += PE_THREADS) {
            const int p = c0 + tid;
            const int gi = p < n ? g[p] : -1;
            int tot;
            const int rk = pe_rank(gi >= 0, s_wave, tot);
            const int pos = s_base + rk;                 // (read behind pe_rank's barriers: thread 0's update of the last chunk is in)
            if (gi >= 0 && pos < cap) pe_write(ev, pos, p, K, gi);
            __syncthreads();                             // every thread has read s_base
            if (tid == 0) s_base += tot;
        }
        __syncthreads();
        const int m = s_base;
        for (int i = min(m, cap) + tid; i < cap; i += PE_THREADS) { ev[3 * i] = -1; ev[3 * i + 1] = -1; ev[3 * i + 2] = -1; }
        if (tid == 0) n_events[v] = m;
        return;
    }
    const unsigned stream_id = (unsigned)draw[v];
    // ---- the number of candidates ----
    int mine = 0;
    for (int p = tid; p < n; p += PE_THREADS) mine += g[p] >= 0 ? 1 : 0;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    if (mine) atomicAdd(&hist[0], (unsigned)mine);
    __syncthreads();
    const int m = (int)hist[0];
    const int r = min(m, cap);
    __syncthreads();
    // ---- radix select of the r-th smallest word (1-based) among the candidates; with m <= cap every candidate survives ----
    unsigned thr_word = 0xFFFFFFFFu;
    int n_eq = m;                                        // survivors among the candidates whose word equals thr_word
    if (m > cap) {
        if (tid == 0) { s_prefix = 0u; s_rank = (unsigned)r; }
        __syncthreads();
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const unsigned himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            const unsigned prefix = s_prefix;
            for (int p = tid; p < n; p += PE_THREADS) {
                if (g[p] < 0) continue;
                const unsigned w = philox_word((unsigned)p, stream_id, SITE_PROP, 0u, k0, k1);
                if ((w & himask) == prefix) atomicAdd(&hist[(w >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned rr = s_rank, b = 0;
                for (; b < 255u; ++b) {                  // walk from the smallest digit up
                    if (hist[b] >= rr) break;
                    rr -= hist[b];
                }
                s_rank = rr;
                s_prefix = prefix | (b << shift);
            }
            __syncthreads();
        }
        thr_word = s_prefix;
        n_eq = (int)s_rank;                              // >= 1: the first n_eq candidates, by position, among the ties at thr_word
    }
    // ---- the survivors' keys into LDS: smaller words from the front, ties at thr_word (in position order) from slot r - 1 down ----
    s_key[tid] = ~0ull;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += PE_THREADS) {
        const int p = c0 + tid;
        const bool cand = p < n && g[p] >= 0;
        const unsigned w = cand ? philox_word((unsigned)p, stream_id, SITE_PROP, 0u, k0, k1) : 0u;
        const bool less = cand && (m <= cap || w < thr_word), eq = cand && m > cap && w == thr_word;
        int tot_less, tot_eq;
        const int rl = pe_rank(less, s_wave, tot_less), rq = pe_rank(eq, s_wave, tot_eq);
        const int pl = s_base + rl, pq = s_eq + rq;      // (read behind pe_rank's barriers: thread 0's update of the last chunk is in)
        const unsigned long long key = ((unsigned long long)w << 32) | (unsigned)p;
        if (less && pl < r) s_key[pl] = key;
        if (eq && pq < n_eq) s_key[r - 1 - pq] = key;
        __syncthreads();                                 // every thread has read s_base and s_eq
        if (tid == 0) { s_base += tot_less; s_eq += tot_eq; }
    }
    __syncthreads();
    // ---- bitonic sort of the PE_THREADS keys, ascending (the unused slots hold the largest key) ----
    for (int k = 2; k <= PE_THREADS; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int other = tid ^ j;
            if (other > tid) {
                const unsigned long long a = s_key[tid], b = s_key[other];
                const bool up = (tid & k) == 0;
                if ((a > b) == up) { s_key[tid] = b; s_key[other] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < cap; i += PE_THREADS) {
        if (i < r) {
            const int p = (int)(unsigned)(s_key[i] & 0xFFFFFFFFull);
            pe_write(ev, i, p, K, g[p]);
        } else {
            ev[3 * i] = -1; ev[3 * i + 1] = -1; ev[3 * i + 2] = -1;
        }
    }
    if (tid == 0) n_events[v] = r;
}

}  // namespace echr

using namespace echr;

extern "C" int echr_tap_targets_batch(const int32_t* row_offset, const int32_t* gt_offset, const int32_t* gt, int32_t V, int32_t T_tot,
                                      int32_t G_tot, int32_t G_max, int32_t K, double iou_threshold, double iou_threshold_good, float* iou,
                                      int32_t* gts_index, float* tap_masks, float* tap_labels, int32_t* good_gt, int32_t* n_good,
                                      void* stream) {
    ECHR_REQUIRE(V >= 1 && V <= ECHR_TARGETS_MAX_VIDEOS, "echr_tap_targets_batch: %d videos outside [1, %d]", V, ECHR_TARGETS_MAX_VIDEOS);
    ECHR_REQUIRE(K >= 1 && K <= ECHR_TARGETS_MAX_K, "echr_tap_targets_batch: K = %d outside [1, %d]", K, ECHR_TARGETS_MAX_K);
    ECHR_REQUIRE(T_tot >= V && (int64_t)T_tot * K < (int64_t)1 << 31, "echr_tap_targets_batch: T_tot = %d rows for %d videos at K = %d (at least one row per video, T_tot * K below 2^31)", T_tot, V, K);
    ECHR_REQUIRE(G_tot >= 0 && G_max >= 0 && G_max <= G_tot, "echr_tap_targets_batch: G_tot = %d, G_max = %d", G_tot, G_max);
    ECHR_REQUIRE(G_max <= ECHR_TARGETS_MAX_GT, "echr_tap_targets_batch: a video with %d ground-truth segments (at most %d)", G_max, ECHR_TARGETS_MAX_GT);
    ECHR_REQUIRE(iou_threshold > 0.0 && iou_threshold_good > 0.0, "echr_tap_targets_batch: thresholds %g / %g must be positive (an anchor outside the mask has IoU 0)", iou_threshold, iou_threshold_good);
    ECHR_REQUIRE(row_offset && gt_offset && (G_tot == 0 || gt), "echr_tap_targets_batch: row_offset, gt_offset and gt are required");
    ECHR_REQUIRE(iou && gts_index && tap_masks && tap_labels && good_gt && n_good, "echr_tap_targets_batch: iou, gts_index, tap_masks, tap_labels, good_gt and n_good are required");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tt_zero_kernel, dim3((V + TT_THREADS - 1) / TT_THREADS), dim3(TT_THREADS), 0, st, n_good, V);
    hipLaunchKernelGGL(tap_targets_kernel, dim3((T_tot + TT_ROWS - 1) / TT_ROWS), dim3(TT_THREADS), 0, st, row_offset, gt_offset, gt, V, T_tot,
                       G_tot, K, (float)iou_threshold, (float)iou_threshold_good, iou, gts_index, tap_masks, tap_labels, good_gt, n_good);
    return check_launch("tap_targets_batch");
}

extern "C" int echr_prop_events_batch(const int32_t* good_gt, const int32_t* row_offset, int32_t V, int32_t T_tot, int32_t K, int32_t cap,
                                      int32_t sampled, uint64_t seed, const int32_t* draw, int32_t* events, int32_t* n_events, void* stream) {
    ECHR_REQUIRE(V >= 1 && V <= ECHR_TARGETS_MAX_VIDEOS, "echr_prop_events_batch: %d videos outside [1, %d]", V, ECHR_TARGETS_MAX_VIDEOS);
    ECHR_REQUIRE(K >= 1 && K <= ECHR_TARGETS_MAX_K, "echr_prop_events_batch: K = %d outside [1, %d]", K, ECHR_TARGETS_MAX_K);
    ECHR_REQUIRE(T_tot >= V && (int64_t)T_tot * K < (int64_t)1 << 31, "echr_prop_events_batch: T_tot = %d rows for %d videos at K = %d (at least one row per video, T_tot * K below 2^31)", T_tot, V, K);
    ECHR_REQUIRE(cap >= 1 && cap <= ECHR_PROP_MAX_SAMPLE, "echr_prop_events_batch: prop_sample_num = %d outside [1, %d]", cap, ECHR_PROP_MAX_SAMPLE);
    ECHR_REQUIRE(sampled == 0 || sampled == 1, "echr_prop_events_batch: sampled = %d (0: every good proposal in order, 1: the sampled list)", sampled);
    ECHR_REQUIRE(good_gt && row_offset && events && n_events, "echr_prop_events_batch: good_gt, row_offset, events and n_events are required");
    ECHR_REQUIRE(!sampled || draw, "echr_prop_events_batch: the sampled list needs draw (one stream id per video)");
    hipLaunchKernelGGL(prop_events_kernel, dim3(V), dim3(PE_THREADS), 0, (hipStream_t)stream, good_gt, row_offset, T_tot, K, cap, sampled,
                       (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), draw, events, n_events);
    return check_launch("prop_events_batch");
}
