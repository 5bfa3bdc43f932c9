// Proposal selection on device: the index outputs of eval_utils.gettop1000 (eval_utils.py:259-287).
//   masked = scores * mask;  thr = the topN-th largest masked value (ties included);  keep (n,k) with n >= k and
//   masked[n,k] >= max(thr, val_thres), enumerated n-major / k-minor:  ind = n, feat = [n-k, n+1], conf = masked[n,k].
// One 1024-thread workgroup: an exact 4-pass (8 bits each) radix select over order-preserving uint32 keys finds thr, then
// an ordered compaction (block prefix sums over 1024-element chunks) writes the lists.  Integer outputs are bit-exact.
// The *_batch entries run the same device code for the V videos of a batch, one workgroup per video in one launch, and a second
// one-workgroup launch concatenates the videos' lists.
#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

__device__ __forceinline__ unsigned order_key(float f) {          // monotone float -> uint map
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// mask == nullptr: the causal mask (n >= k ? 1 : 0) is generated in place of the load; the product is formed either way, so the keys are
// those of the explicit mask.
__device__ __forceinline__ float masked_score(const float* __restrict__ scores, const float* __restrict__ mask, long i, int K) {
    return scores[i] * (mask ? mask[i] : ((int)(i / K) >= (int)(i % K) ? 1.f : 0.f));
}

// The selection of ONE score grid by the calling 1024-thread workgroup; returns the number of entries written (to every thread).
// out_ind may be nullptr (ind = feat[1] - 1).
__device__ int select_threshold(const float* __restrict__ scores, const float* __restrict__ mask, int T, int K, int topN, float val_thres,
                                int* __restrict__ out_ind, int* __restrict__ out_feat, float* __restrict__ out_conf) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_rank;
    __shared__ int s_scan[1024];
    __shared__ int s_base;
    const long n = (long)T * K;
    const int tid = threadIdx.x;
    // ---- radix select of the r-th largest key, r = min(n, topN) (1-based) ----
    if (tid == 0) { s_prefix = 0u; s_rank = (unsigned)min((long)topN, n); }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = s_prefix;
        for (long i = tid; i < n; i += 1024) {
            const unsigned key = order_key(masked_score(scores, mask, i, K));
            if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned r = s_rank, b = 255;
            for (;; --b) {                          // walk from the largest digit down
                if (hist[b] >= r) break;
                r -= hist[b];
                if (b == 0) break;
            }
            s_rank = r;
            s_prefix = prefix | (b << shift);
        }
        __syncthreads();
    }
    const unsigned thr_key = max(s_prefix, order_key(val_thres));
    // ---- ordered compaction ----
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (long c0 = 0; c0 < n; c0 += 1024) {
        const long i = c0 + tid;
        int flag = 0, row = 0, col = 0;
        float v = 0.f;
        if (i < n) {
            row = (int)(i / K); col = (int)(i % K);
            v = masked_score(scores, mask, i, K);
            flag = (row >= col && order_key(v) >= thr_key) ? 1 : 0;
        }
        s_scan[tid] = flag;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {      // inclusive Hillis-Steele scan
            const int add = tid >= off ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        if (flag) {
            const int pos = s_base + s_scan[tid] - 1;
            if (out_ind) out_ind[pos] = row;
            out_feat[2 * pos] = row - col;
            out_feat[2 * pos + 1] = row + 1;
            out_conf[pos] = v;
        }
        __syncthreads();
        if (tid == 1023) s_base += s_scan[1023];
        __syncthreads();
    }
    return s_base;          // (stable: the loop's last barrier follows the last update)
}

__global__ __launch_bounds__(1024) void top_proposals_kernel(const float* __restrict__ scores, const float* __restrict__ mask, int T, int K,
                                                             int topN, float val_thres, int* __restrict__ out_ind,
                                                             int* __restrict__ out_feat, float* __restrict__ out_conf,
                                                             int* __restrict__ out_count) {
    const int m = select_threshold(scores, mask, T, K, topN, val_thres, out_ind, out_feat, out_conf);
    if (threadIdx.x == 0) out_count[0] = m;
}

// Multi-video batches: workgroup v selects over the rows [row_offset[v], row_offset[v+1]) of the concatenated grid -- n and k local to the
// video -- and leaves its lists at entry row_offset[v]*K of the output buffers (a video cannot write more than its T_v*K cells, so the
// regions are disjoint); compact_proposals_kernel then closes the gaps.  A video whose offsets fall outside [0, T_tot] selects nothing.
__global__ __launch_bounds__(1024) void top_proposals_batch_kernel(const float* __restrict__ scores, const float* __restrict__ mask,
                                                                   const int* __restrict__ row_offset, int T_tot, int K, int topN,
                                                                   float val_thres, int* __restrict__ feat, float* __restrict__ conf,
                                                                   int* __restrict__ count) {
    const int v = blockIdx.x, r0 = row_offset[v], r1 = row_offset[v + 1];
    int m = 0;
    if (r0 >= 0 && r1 > r0 && r1 <= T_tot) {          // (uniform over the workgroup)
        const long o = (long)r0 * K;
        m = select_threshold(scores + o, mask ? mask + o : nullptr, r1 - r0, K, topN, val_thres, nullptr, feat + 2 * o, conf + o);
    }
    if (threadIdx.x == 0) count[v] = m;
}

// Greedy 1-D non-maximum suppression (eval_utils.gettop1000_nms, eval_utils.py:290-331).  Candidates (n, k < min(n, K)) = segments
// [n-k, n+1]; repeat up to topN times: pick the best live candidate (ties -> the later one in n-major order, i.e. the last element
// of a stable ascending sort), kill every live candidate whose inclusive temporal IoU with it exceeds `overlap`.  IoU in float64
// with the reference's operation order (wh / (area_i + area_j - wh)), so the comparison against `overlap` is bit-identical.
// `live` is a [T*K] float scratch: the score while the candidate is live, -inf otherwise.
// One grid by the calling 1024-thread workgroup; returns the number of picks (to every thread).
__device__ int select_nms(const float* __restrict__ scores, int T, int K, int topN, double overlap, float* __restrict__ live,
                          int* __restrict__ out_feat, float* __restrict__ out_conf) {
    __shared__ float s_val[16];
    __shared__ int s_idx[16];
    __shared__ int s_pick;
    const long n = (long)T * K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long i = tid; i < n; i += 1024) {
        const int row = (int)(i / K), col = (int)(i % K);
        live[i] = col < min(row, K) ? scores[i] : -INFINITY;
    }
    __syncthreads();
    int picked = 0;
    for (; picked < topN; ++picked) {
        float bv = -INFINITY;
        int bi = -1;
        for (long i = tid; i < n; i += 1024) {
            const float v = live[i];
            if (v > bv || (v == bv && v != -INFINITY)) { bv = v; bi = (int)i; }        // ascending i: ties keep the larger index
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi > bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_val[wave] = bv; s_idx[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            float v = s_val[0]; int ix = s_idx[0];
            for (int w = 1; w < 16; ++w) if (s_val[w] > v || (s_val[w] == v && s_idx[w] > ix)) { v = s_val[w]; ix = s_idx[w]; }
            s_pick = (v == -INFINITY) ? -1 : ix;
            if (s_pick >= 0) {
                const int row = ix / K, col = ix % K;
                out_feat[2 * picked] = row - col;
                out_feat[2 * picked + 1] = row + 1;
                out_conf[picked] = v;
            }
        }
        __syncthreads();
        const int pk = s_pick;
        if (pk < 0) break;
        const int prow = pk / K, pcol = pk % K;
        const double pt1 = prow - pcol, pt2 = prow + 1, parea = pt2 - pt1 + 1.0;
        for (long i = tid; i < n; i += 1024) {
            if (live[i] == -INFINITY) continue;
            const int row = (int)(i / K), col = (int)(i % K);
            const double t1 = row - col, t2 = row + 1;
            const double wh = fmax(0.0, fmin(pt2, t2) - fmax(pt1, t1) + 1.0);
            const double o = wh / (parea + (t2 - t1 + 1.0) - wh);
            if (i == pk || !(o <= overlap)) live[i] = -INFINITY;
        }
        __syncthreads();
    }
    return picked;
}

__global__ __launch_bounds__(1024) void top_proposals_nms_kernel(const float* __restrict__ scores, int T, int K, int topN, double overlap,
                                                                 float* __restrict__ live, int* __restrict__ out_feat,
                                                                 float* __restrict__ out_conf, int* __restrict__ out_count) {
    const int m = select_nms(scores, T, K, topN, overlap, live, out_feat, out_conf);
    if (threadIdx.x == 0) out_count[0] = m;
}

// Multi-video batches: workgroup v runs the greedy NMS over its own rows and leaves its picks at entry v*topN of the output buffers.
__global__ __launch_bounds__(1024) void top_proposals_nms_batch_kernel(const float* __restrict__ scores, const int* __restrict__ row_offset,
                                                                       int T_tot, int K, int topN, double overlap, float* __restrict__ live,
                                                                       int* __restrict__ feat, float* __restrict__ conf,
                                                                       int* __restrict__ count) {
    const int v = blockIdx.x, r0 = row_offset[v], r1 = row_offset[v + 1];
    int m = 0;
    if (r0 >= 0 && r1 > r0 && r1 <= T_tot) {
        const long o = (long)r0 * K, p = (long)v * topN;
        m = select_nms(scores + o, r1 - r0, K, topN, overlap, live + o, feat + 2 * p, conf + p);
    }
    if (threadIdx.x == 0) count[v] = m;
}

// Second launch of both batched entries, one workgroup: the exclusive scan of the V counts, then video by video the move of its list from
// its staging entry (row_offset[v]*K, or v*stride when stride > 0) to event_offset[v].  In place: a video's destination never lies
// behind its source nor reaches into the next video's source, and inside a video every 1024-entry chunk is read, then -- after a barrier
// -- written.  `cap`: entries the buffers hold.  The batch-absolute copies, vid, the total and the largest interval length are produced on the way.
__global__ __launch_bounds__(1024) void compact_proposals_kernel(const int* __restrict__ row_offset, int V, int K, int stride, long cap,
                                                                 int* __restrict__ count, int* __restrict__ event_offset,
                                                                 int* __restrict__ vid, int* __restrict__ ind, int* feat,
                                                                 int* __restrict__ ind_abs, int* __restrict__ feat_abs, float* conf) {
    __shared__ int s_maxlen;
    const int tid = threadIdx.x;
    if (tid == 0) s_maxlen = 0;
    __syncthreads();
    long dst0 = 0;
    int maxlen = 0;
    for (int v = 0; v < V; ++v) {
        const int r0 = row_offset[v];
        const int c = dst0 + count[v] <= cap ? count[v] : 0;          // (malformed offsets only: never write past the caller's capacity)
        const long src0 = stride > 0 ? (long)v * stride : (long)r0 * K;
        if (tid == 0) event_offset[v] = (int)dst0;
        for (int c0 = 0; c0 < c; c0 += 1024) {
            const int i = c0 + tid;
            int s = 0, e = 0;
            float cf = 0.f;
            if (i < c) { s = feat[2 * (src0 + i)]; e = feat[2 * (src0 + i) + 1]; cf = conf[src0 + i]; }
            __syncthreads();
            if (i < c) {
                const long d = dst0 + i;
                feat[2 * d] = s; feat[2 * d + 1] = e; conf[d] = cf;
                ind[d] = e - 1;
                feat_abs[2 * d] = s + r0; feat_abs[2 * d + 1] = e + r0;
                ind_abs[d] = e - 1 + r0;
                vid[d] = v;
                maxlen = max(maxlen, e - s);
            }
            __syncthreads();
        }
        dst0 += c;
    }
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();
    if (tid == 0) { event_offset[V] = (int)dst0; count[V] = (int)dst0; count[V + 1] = s_maxlen; }
}

}  // namespace echr

using namespace echr;

extern "C" int echr_top_proposals_nms(const float* scores, int32_t T, int32_t K, int32_t topN, double overlap, float* scratch,
                                      int32_t* out_feat, float* out_conf, int32_t* out_count, void* stream) {
    ECHR_REQUIRE(scores && scratch && out_feat && out_conf && out_count && T > 0 && K > 0 && topN > 0, "top_proposals_nms: bad arguments");
    hipLaunchKernelGGL(top_proposals_nms_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, scores, T, K, topN, overlap, scratch, out_feat,
                       out_conf, out_count);
    return check_launch("top_proposals_nms");
}


extern "C" int echr_top_proposals(const float* scores, const float* mask, int32_t T, int32_t K, int32_t topN, float val_thres,
                                  int32_t* out_ind, int32_t* out_feat, float* out_conf, int32_t* out_count, void* stream) {
    ECHR_REQUIRE(scores && mask && out_ind && out_feat && out_conf && out_count && T > 0 && K > 0 && topN > 0, "top_proposals: bad arguments");
    hipLaunchKernelGGL(top_proposals_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, scores, mask, T, K, topN, val_thres, out_ind, out_feat,
                       out_conf, out_count);
    return check_launch("top_proposals");
}

/* the second launch shared by the two batched entries */
static int launch_compact(const char* who, const int32_t* row_offset, int32_t V, int32_t K, int32_t stride, long cap, int32_t* count, int32_t* event_offset,
                          int32_t* vid, int32_t* ind, int32_t* feat, int32_t* ind_abs, int32_t* feat_abs, float* conf, hipStream_t st) {
    hipLaunchKernelGGL(compact_proposals_kernel, dim3(1), dim3(1024), 0, st, row_offset, V, K, stride, cap, count, event_offset, vid, ind, feat,
                       ind_abs, feat_abs, conf);
    return check_launch(who);
}

extern "C" int echr_top_proposals_batch(const float* scores, const float* mask, const int32_t* row_offset, int32_t T_tot, int32_t V, int32_t K,
                                        int32_t topN, float val_thres, int32_t* count, int32_t* event_offset, int32_t* vid, int32_t* ind,
                                        int32_t* feat, int32_t* ind_abs, int32_t* feat_abs, float* conf, void* stream) {
    ECHR_REQUIRE(scores && row_offset && count && event_offset && vid && ind && feat && ind_abs && feat_abs && conf && T_tot > 0 && V > 0 &&
                 V <= T_tot && K > 0 && topN > 0 && (long)T_tot * K < 0x7FFFFFFFL, "top_proposals_batch: bad arguments");
    hipLaunchKernelGGL(top_proposals_batch_kernel, dim3(V), dim3(1024), 0, (hipStream_t)stream, scores, mask, row_offset, T_tot, K, topN, val_thres,
                       feat, conf, count);
    const int rc = check_launch("top_proposals_batch");
    return rc ? rc : launch_compact("top_proposals_batch", row_offset, V, K, 0, (long)T_tot * K, count, event_offset, vid, ind, feat, ind_abs, feat_abs, conf,
                                    (hipStream_t)stream);
}

extern "C" int echr_top_proposals_nms_batch(const float* scores, const int32_t* row_offset, int32_t T_tot, int32_t V, int32_t K, int32_t topN,
                                            double overlap, float* live, int32_t* count, int32_t* event_offset, int32_t* vid, int32_t* ind,
                                            int32_t* feat, int32_t* ind_abs, int32_t* feat_abs, float* conf, void* stream) {
    ECHR_REQUIRE(scores && row_offset && live && count && event_offset && vid && ind && feat && ind_abs && feat_abs && conf && T_tot > 0 && V > 0 &&
                 V <= T_tot && K > 0 && topN > 0 && (long)T_tot * K < 0x7FFFFFFFL && (long)V * topN < 0x3FFFFFFFL,
                 "top_proposals_nms_batch: bad arguments");
    hipLaunchKernelGGL(top_proposals_nms_batch_kernel, dim3(V), dim3(1024), 0, (hipStream_t)stream, scores, row_offset, T_tot, K, topN, overlap,
                       live, feat, conf, count);
    const int rc = check_launch("top_proposals_nms_batch");
    return rc ? rc : launch_compact("top_proposals_nms_batch", row_offset, V, K, topN, (long)V * topN, count, event_offset, vid, ind, feat, ind_abs, feat_abs, conf,
                                    (hipStream_t)stream);
}
