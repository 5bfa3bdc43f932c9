// Dense-caption scoring over token ids (echr_densecap_*): the ANETcaptions protocol without METEOR.
//   match       a thread per prediction / per ground truth: partner counts and strict-cover flags at every threshold, no atomics
//   fill        a thread per (threshold, prediction): its pairs, behind the exclusive scan of the counts
//   pair_stats  a wave per pair, lane j holding token j of the candidate and of the reference: LCS by the bit-vector recurrence on
//               wave ballots, clipped n-gram matches on section 4s's exact keys
//   reduce      a workgroup per (video, threshold): integer sums (exact, order-free), BLEU in fp64, the ROUGE-L / CIDEr-D means summed
//               serially in pair order; then the means over the videos in video order
// The IoU is fp64 in one written order with no multiply next to an add, so nothing can be contracted: its bits are the host's.
#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

constexpr int DC_MAX_L = 63;
constexpr int DC_MAX_TAU = ECHR_DENSECAP_MAX_TAU;
constexpr int DC_STATS = ECHR_DENSECAP_STATS;
constexpr int DC_VCOLS = ECHR_DENSECAP_VIDEO_COLS;
constexpr int DC_MCOLS = ECHR_DENSECAP_MEAN_COLS;
constexpr int DC_MAX_TOK = 65534;                   // tok + 1 fits a 16-bit key field
constexpr int DC_THREADS = 256;
constexpr int DC_SUMS = 13;                         // match_1..4, guess_1..4, c, r, strict-covered predictions, unmatched, covered ground truths

__device__ __forceinline__ double dc_iou(double s1, double e1, double s2, double e2) {
    const double inter = fmax(0.0, fmin(e1, e2) - fmax(s1, s2));
    const double uni = fmin(fmax(e1, e2) - fmin(s1, s2), (e2 - s2) + (e1 - s1));
    return inter / (uni + 1e-8);
}

// the video that owns row i: the first v with off[v + 1] > i
__device__ __forceinline__ int dc_video_of(const int32_t* __restrict__ off, int V, int i) {
    int lo = 0, hi = V;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    return min(lo, V - 1);
}

__device__ __forceinline__ int dc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(DC_THREADS) void dc_match_kernel(const echr_densecap_args a) {
    const int i = blockIdx.x * DC_THREADS + threadIdx.x;
    if (i >= a.N_tot + a.G_tot) return;
    double tau[DC_MAX_TAU];
#pragma unroll
    for (int k = 0; k < DC_MAX_TAU; ++k) tau[k] = k < a.n_tau ? a.tau[k] : 0.0;
    int cnt[DC_MAX_TAU], hit[DC_MAX_TAU];
#pragma unroll
    for (int k = 0; k < DC_MAX_TAU; ++k) cnt[k] = hit[k] = 0;
    if (i < a.N_tot) {
        const int v = dc_video_of(a.pred_offset, a.V, i);
        const int g0 = dc_clamp(a.gt_offset[v], 0, a.G_tot), g1 = dc_clamp(a.gt_offset[v + 1], g0, a.G_tot);
        const double s1 = a.pred_stamps[2 * (int64_t)i], e1 = a.pred_stamps[2 * (int64_t)i + 1];
        for (int g = g0; g < g1; ++g) {
            const double iou = dc_iou(s1, e1, a.gt_stamps[2 * (int64_t)g], a.gt_stamps[2 * (int64_t)g + 1]);
#pragma unroll
            for (int k = 0; k < DC_MAX_TAU; ++k) {
                cnt[k] += iou >= tau[k];
                hit[k] |= iou > tau[k];
            }
        }
#pragma unroll
        for (int k = 0; k < DC_MAX_TAU; ++k)
            if (k < a.n_tau) {
                a.count[(int64_t)k * a.N_tot + i] = max(cnt[k], 1);
                a.pred_flag[(int64_t)k * a.N_tot + i] = hit[k] | (cnt[k] == 0 ? 2 : 0);
            }
    } else {
        const int j = i - a.N_tot;
        const int v = dc_video_of(a.gt_offset, a.V, j);
        const int p0 = dc_clamp(a.pred_offset[v], 0, a.N_tot), p1 = dc_clamp(a.pred_offset[v + 1], p0, a.N_tot);
        const double s2 = a.gt_stamps[2 * (int64_t)j], e2 = a.gt_stamps[2 * (int64_t)j + 1];
        for (int p = p0; p < p1; ++p) {
            const double iou = dc_iou(a.pred_stamps[2 * (int64_t)p], a.pred_stamps[2 * (int64_t)p + 1], s2, e2);
#pragma unroll
            for (int k = 0; k < DC_MAX_TAU; ++k) hit[k] |= iou > tau[k];
        }
#pragma unroll
        for (int k = 0; k < DC_MAX_TAU; ++k)
            if (k < a.n_tau) a.gt_hit[(int64_t)k * a.G_tot + j] = hit[k];
    }
}

__global__ __launch_bounds__(DC_THREADS) void dc_fill_kernel(const echr_densecap_args a) {
    const int64_t idx = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    if (idx >= (int64_t)a.n_tau * a.N_tot) return;
    const int k = (int)(idx / a.N_tot), i = (int)(idx % a.N_tot);
    const int64_t pos = a.start[idx];
    const int64_t n = min(a.start[idx + 1], a.P_tot) - pos;          // never write past the buffers, whatever the scan holds
    if (pos < 0 || n <= 0) return;
    const double tau = a.tau[k];
    const int v = dc_video_of(a.pred_offset, a.V, i);
    const int g0 = dc_clamp(a.gt_offset[v], 0, a.G_tot), g1 = dc_clamp(a.gt_offset[v + 1], g0, a.G_tot);
    const double s1 = a.pred_stamps[2 * (int64_t)i], e1 = a.pred_stamps[2 * (int64_t)i + 1];
    int64_t w = 0;
    for (int g = g0; g < g1 && w < n; ++g)
        if (dc_iou(s1, e1, a.gt_stamps[2 * (int64_t)g], a.gt_stamps[2 * (int64_t)g + 1]) >= tau) {
            a.pair_pred[pos + w] = i;
            a.pair_gt[pos + w] = g;
            ++w;
        }
    if (w == 0) {
        a.pair_pred[pos] = i;
        a.pair_gt[pos] = -1;
    }
}

__device__ __forceinline__ int dc_token(long long v) { return (int)(v < 0 ? 0 : (v > DC_MAX_TOK ? DC_MAX_TOK : v)); }

__device__ __forceinline__ int dc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one wave (= one workgroup) per pair
__global__ __launch_bounds__(64) void dc_pair_kernel(const echr_densecap_args a) {
    __shared__ int s_c[64 + 4], s_r[64 + 4];
    __shared__ uint64_t s_kc[64], s_kr[64];
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const int ip = a.pair_pred[p], ig = a.pair_gt[p];
    int tc = 0, tr = 0;
    if (lane < a.T && ip >= 0 && ip < a.N_tot) {
        const int64_t at = (int64_t)ip * a.ld + (int64_t)lane * a.cs;
        tc = dc_token(a.cand_i32 ? (long long)((const int32_t*)a.cand)[at] : (long long)((const int64_t*)a.cand)[at]);
    }
    if (lane < a.L && ig >= 0 && ig < a.G_tot) tr = dc_token(a.refs[(int64_t)ig * a.L + lane]);
    // T, L <= 63: lane 63 always holds a 0, so both ballots have a bit set
    const int len_c = __ffsll((long long)__ballot(tc == 0)) - 1;
    const int len_r = __ffsll((long long)__ballot(tr == 0)) - 1;
    s_c[lane] = tc;
    s_r[lane] = tr;
    if (lane < 4) s_c[64 + lane] = s_r[64 + lane] = 0;
    __syncthreads();
    // LCS: bit j of W is 0 where the LCS grows at reference position j (Crochemore et al. / Hyyro's recurrence)
    unsigned long long W = ~0ull;
    for (int i = 0; i < len_c; ++i) {
        const int ci = s_c[i];
        const unsigned long long M = __ballot(lane < len_r && tr == ci);
        W = (W + (W & M)) | (W & ~M);
    }
    const int lcs = __popcll(~W & ((1ull << len_r) - 1ull));
    int match[4];
    const int jmax = max(len_c, len_r);
#pragma unroll
    for (int n = 1; n <= 4; ++n) {
        const bool valid = lane + n <= len_c;
        uint64_t key = 0, kr = 0;
        if (valid)
            for (int k = 0; k < n; ++k) key |= (uint64_t)(s_c[lane + k] + 1) << (16 * k);
        if (lane + n <= len_r)
            for (int k = 0; k < n; ++k) kr |= (uint64_t)(s_r[lane + k] + 1) << (16 * k);
        __syncthreads();          // the previous order's reads are done
        s_kc[lane] = key;
        s_kr[lane] = kr;
        __syncthreads();
        int tfc = 0, tfr = 0;
        bool first = true;
        for (int j = 0; j < jmax; ++j) {          // a position without an n-gram holds key 0, which no n-gram has
            const bool eq = s_kc[j] == key;
            tfc += eq;
            first = first && !(eq && j < lane);
            tfr += s_kr[j] == key;
        }
        match[n - 1] = dc_wave_sum(valid && first ? min(tfc, tfr) : 0);
    }
    if (lane == 0) {
        const int lr = ig >= 0 ? len_r : 1;          // the unmatched pair: reference length 1, nothing matches
        int32_t* o = a.stats + p * DC_STATS;
        o[0] = match[0]; o[1] = match[1]; o[2] = match[2]; o[3] = match[3];
        o[4] = len_c; o[5] = lr; o[6] = lcs;
        double rg = 0.0;
        if (lcs > 0) {          // then len_c and len_r are positive too
            const double P = (double)lcs / (double)len_c, R = (double)lcs / (double)lr, b2 = 1.2 * 1.2;
            rg = (1.0 + b2) * P * R / (R + b2 * P);
        }
        a.rouge[p] = rg;
    }
}

__global__ __launch_bounds__(DC_THREADS) void dc_reduce_kernel(const echr_densecap_args a) {
    __shared__ long long s_part[DC_SUMS][DC_THREADS];
    __shared__ long long s_sum[DC_SUMS];
    __shared__ double s_mean[2];
    const int v = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int p0 = dc_clamp(a.pred_offset[v], 0, a.N_tot), p1 = dc_clamp(a.pred_offset[v + 1], p0, a.N_tot);
    const int g0 = dc_clamp(a.gt_offset[v], 0, a.G_tot), g1 = dc_clamp(a.gt_offset[v + 1], g0, a.G_tot);
    const int64_t b = min(max(a.start[(int64_t)k * a.N_tot + p0], (int64_t)0), a.P_tot);
    const int64_t e = min(max(a.start[(int64_t)k * a.N_tot + p1], b), a.P_tot);
    long long acc[DC_SUMS];
#pragma unroll
    for (int j = 0; j < DC_SUMS; ++j) acc[j] = 0;
    if (a.stats)
        for (int64_t p = b + tid; p < e; p += DC_THREADS) {
            const int32_t* s = a.stats + p * DC_STATS;
            const int lc = s[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                acc[n] += s[n];
                acc[4 + n] += max(lc - n, 0);          // order n + 1: len_c - (n + 1) + 1 n-grams
            }
            acc[8] += lc;
            acc[9] += s[5];
        }
    for (int i = p0 + tid; i < p1; i += DC_THREADS) {
        const int f = a.pred_flag[(int64_t)k * a.N_tot + i];
        acc[10] += f & 1;
        acc[11] += (f >> 1) & 1;
    }
    for (int j = g0 + tid; j < g1; j += DC_THREADS) acc[12] += a.gt_hit[(int64_t)k * a.G_tot + j] != 0;
#pragma unroll
    for (int j = 0; j < DC_SUMS; ++j) s_part[j][tid] = acc[j];
    __syncthreads();
    if (tid < DC_SUMS) {
        long long s = 0;
        for (int t = 0; t < DC_THREADS; ++t) s += s_part[tid][t];
        s_sum[tid] = s;
    }
    // the two means, each summed by one thread (of its own wave) in pair order
    if (tid == 64 || tid == 128) {
        double s = 0.0;
        if (a.stats && e > b) {
            if (tid == 64) {
                for (int64_t p = b; p < e; ++p) s += a.rouge[p];
            } else if (a.cider) {
                for (int64_t p = b; p < e; ++p) s += (double)a.cider[p];
            }
            s /= (double)(e - b);
        }
        s_mean[tid == 64 ? 0 : 1] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double* o = a.video + ((int64_t)k * a.V + v) * DC_VCOLS;
        const int P = p1 - p0, G = g1 - g0;
        o[0] = G > 0 ? (double)s_sum[12] / (double)G : 0.0;
        o[1] = P > 0 ? (double)s_sum[10] / (double)P : 0.0;
        double bleu[4] = {0.0, 0.0, 0.0, 0.0};
        if (a.stats && e > b) {
            const double ratio = ((double)s_sum[8] + 1e-15) / ((double)s_sum[9] + 1e-9);
            const double bp = ratio >= 1.0 ? 1.0 : exp(1.0 - 1.0 / ratio);
            double prod = 1.0;
            for (int n = 0; n < 4; ++n) {
                prod *= ((double)s_sum[n] + 1e-15) / ((double)s_sum[4 + n] + 1e-9);
                bleu[n] = pow(prod, 1.0 / (double)(n + 1)) * bp;
            }
        }
        o[2] = bleu[0]; o[3] = bleu[1]; o[4] = bleu[2]; o[5] = bleu[3];
        o[6] = s_mean[0];
        o[7] = s_mean[1];
        o[8] = (double)(e - b);
        o[9] = (double)s_sum[11];
    }
}

// mean[k, c] over the videos, in video order
__global__ __launch_bounds__(64) void dc_mean_kernel(const echr_densecap_args a) {
    const int t = threadIdx.x;
    if (t >= a.n_tau * DC_MCOLS) return;
    const int k = t / DC_MCOLS, c = t % DC_MCOLS;
    double s = 0.0;
    for (int v = 0; v < a.V; ++v) s += a.video[((int64_t)k * a.V + v) * DC_VCOLS + c];
    a.mean[k * DC_MCOLS + c] = s / (double)a.V;
}

static int dc_check_sizes(const echr_densecap_args* a, const char* who) {
    ECHR_REQUIRE(a != nullptr, "%s: null arguments", who);
    ECHR_REQUIRE(a->V >= 0 && a->N_tot >= 0 && a->G_tot >= 0, "%s: negative sizes (V = %d, N_tot = %d, G_tot = %d)", who, a->V, a->N_tot, a->G_tot);
    ECHR_REQUIRE(a->n_tau >= 1 && a->n_tau <= DC_MAX_TAU, "%s: %d thresholds outside [1, %d]", who, a->n_tau, DC_MAX_TAU);
    ECHR_REQUIRE((int64_t)a->n_tau * a->N_tot < (1ll << 31) && (int64_t)a->N_tot + a->G_tot < (1ll << 31), "%s: too many rows", who);
    return 0;
}

static int dc_check_events(const echr_densecap_args* a, const char* who) {
    ECHR_REQUIRE(a->pred_offset && a->gt_offset && a->tau, "%s: pred_offset, gt_offset and tau are required", who);
    ECHR_REQUIRE((a->N_tot == 0 || a->pred_stamps) && (a->G_tot == 0 || a->gt_stamps), "%s: the events need their stamps", who);
    return 0;
}

static int dc_check_pairs(const echr_densecap_args* a, const char* who) {
    ECHR_REQUIRE(a->P_tot >= 0 && a->P_tot < (1ll << 31), "%s: %lld pairs outside [0, 2^31)", who, (long long)a->P_tot);
    return 0;
}

}  // namespace echr

using namespace echr;

extern "C" int echr_densecap_match(const echr_densecap_args* a, void* stream) {
    if (int rc = dc_check_sizes(a, "echr_densecap_match")) return rc;
    if (a->V == 0 || a->N_tot + a->G_tot == 0) return 0;
    if (int rc = dc_check_events(a, "echr_densecap_match")) return rc;
    ECHR_REQUIRE((a->N_tot == 0 || (a->count && a->pred_flag)) && (a->G_tot == 0 || a->gt_hit), "echr_densecap_match: count, pred_flag and gt_hit are required");
    const int rows = a->N_tot + a->G_tot;
    hipLaunchKernelGGL(dc_match_kernel, dim3((rows + DC_THREADS - 1) / DC_THREADS), dim3(DC_THREADS), 0, (hipStream_t)stream, *a);
    return check_launch("densecap_match");
}

extern "C" int echr_densecap_fill(const echr_densecap_args* a, void* stream) {
    if (int rc = dc_check_sizes(a, "echr_densecap_fill")) return rc;
    if (int rc = dc_check_pairs(a, "echr_densecap_fill")) return rc;
    if (a->V == 0 || a->N_tot == 0 || a->P_tot == 0) return 0;
    if (int rc = dc_check_events(a, "echr_densecap_fill")) return rc;
    ECHR_REQUIRE(a->start && a->pair_pred && a->pair_gt, "echr_densecap_fill: start, pair_pred and pair_gt are required");
    const int64_t rows = (int64_t)a->n_tau * a->N_tot;
    hipLaunchKernelGGL(dc_fill_kernel, dim3((unsigned)((rows + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, (hipStream_t)stream, *a);
    return check_launch("densecap_fill");
}

extern "C" int echr_densecap_pair_stats(const echr_densecap_args* a, void* stream) {
    if (int rc = dc_check_sizes(a, "echr_densecap_pair_stats")) return rc;
    if (int rc = dc_check_pairs(a, "echr_densecap_pair_stats")) return rc;
    ECHR_REQUIRE(a->L >= 1 && a->L <= DC_MAX_L, "echr_densecap_pair_stats: seq_length %d outside [1, %d]", a->L, DC_MAX_L);
    ECHR_REQUIRE(a->T >= 0 && a->T <= DC_MAX_L, "echr_densecap_pair_stats: width %d outside [0, %d]", a->T, DC_MAX_L);
    if (a->P_tot == 0) return 0;
    ECHR_REQUIRE(a->pair_pred && a->pair_gt && a->stats && a->rouge, "echr_densecap_pair_stats: pair_pred, pair_gt, stats and rouge are required");
    ECHR_REQUIRE((a->T == 0 || a->cand) && (a->G_tot == 0 || a->refs), "echr_densecap_pair_stats: cand and refs are required");
    hipLaunchKernelGGL(dc_pair_kernel, dim3((unsigned)a->P_tot), dim3(64), 0, (hipStream_t)stream, *a);
    return check_launch("densecap_pair_stats");
}

extern "C" int echr_densecap_reduce(const echr_densecap_args* a, void* stream) {
    if (int rc = dc_check_sizes(a, "echr_densecap_reduce")) return rc;
    if (int rc = dc_check_pairs(a, "echr_densecap_reduce")) return rc;
    if (a->V == 0) return 0;
    ECHR_REQUIRE(a->V <= 65535, "echr_densecap_reduce: %d videos (at most 65535 per call)", a->V);
    ECHR_REQUIRE(a->pred_offset && a->gt_offset, "echr_densecap_reduce: pred_offset and gt_offset are required");
    ECHR_REQUIRE(a->start && (a->N_tot == 0 || a->pred_flag) && (a->G_tot == 0 || a->gt_hit), "echr_densecap_reduce: start, pred_flag and gt_hit are required");
    ECHR_REQUIRE(a->stats == nullptr || a->rouge, "echr_densecap_reduce: stats come with rouge");
    ECHR_REQUIRE(a->video && a->mean, "echr_densecap_reduce: video and mean are required");
    hipLaunchKernelGGL(dc_reduce_kernel, dim3(a->V, a->n_tau), dim3(DC_THREADS), 0, (hipStream_t)stream, *a);
    if (int rc = check_launch("densecap_reduce")) return rc;
    hipLaunchKernelGGL(dc_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a);
    return check_launch("densecap_mean");
}
