// Beam search over the launch-per-step decode chain (echr_decoder_beam, driver in decoder.hip): the per-step selection kernel and the
// finalize kernel.  Event n's B slots are rows n*B + j of the chain; one workgroup per event and step.
//
// Semantics: candidates s_j + logp_j[v] over the alive slots j and every token v, the B largest win, ties to the
// smaller j then the smaller v; new slot k is the k-th winner and takes its parent's LSTM state and history.  A winner with v == 0, or any
// winner at the last step, is a finished hypothesis; the event's result is replaced only by a finished one with a strictly greater score
// (the first one is always taken), the smaller k offered first.
#include <climits>
#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

constexpr int BEAM_MAX = 16;

// (c, v) ranks before (oc, ov): larger score, then smaller index
__device__ __forceinline__ bool beam_before(float c, int v, float oc, int ov) { return c > oc || (c == oc && v < ov); }

// the row's top-B (candidate score, token, log-prob) for slot score sj, in rank order, written by lane 0 to oc / ov / olp.
// EPW > 0: the row is held in registers (V1 <= 64 EPW); 0: any V1, re-read from memory in every round.
template <int EPW>
__device__ void beam_row_topb(const float* __restrict__ x, int V1, int B, float sj, int lane, float* oc, int* ov, float* olp) {
    float rv[EPW > 0 ? EPW : 1];
    float m = -INFINITY;
    if (EPW > 0) {
#pragma unroll
        for (int i = 0; i < EPW; ++i) { const int j = lane + 64 * i; rv[i] = j < V1 ? x[j] : -INFINITY; m = fmaxf(m, rv[i]); }
    } else {
        for (int j = lane; j < V1; j += 64) m = fmaxf(m, x[j]);
    }
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float s = 0.f;
    if (EPW > 0) {
#pragma unroll
        for (int i = 0; i < EPW; ++i) if (lane + 64 * i < V1) s += expf(rv[i] - m);
    } else {
        for (int j = lane; j < V1; j += 64) s += expf(x[j] - m);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float ls = logf(s);                 // log-softmax: logp_v = (x_v - m) - ls (exact 0 - ls at the maximum, as the greedy step)
    // B rounds: round r finds the best candidate ranked after round r-1's
    float pc = INFINITY;
    int pv = -1;
    for (int r = 0; r < B; ++r) {
        float bc = -INFINITY, blp = -INFINITY;
        int bv = INT_MAX;
        if (EPW > 0) {
#pragma unroll
            for (int i = 0; i < EPW; ++i) {
                const int j = lane + 64 * i;
                const float lp = (rv[i] - m) - ls, c = sj + lp;
                if (j < V1 && beam_before(c, j, bc, bv) && beam_before(pc, pv, c, j)) { bc = c; bv = j; blp = lp; }
            }
        } else {
            for (int j = lane; j < V1; j += 64) {
                const float lp = (x[j] - m) - ls, c = sj + lp;
                if (beam_before(c, j, bc, bv) && beam_before(pc, pv, c, j)) { bc = c; bv = j; blp = lp; }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float c2 = __shfl_xor(bc, off, 64), l2 = __shfl_xor(blp, off, 64);
            const int v2 = __shfl_xor(bv, off, 64);
            if (beam_before(c2, v2, bc, bv)) { bc = c2; bv = v2; blp = l2; }
        }
        if (lane == 0) { oc[r] = bc; ov[r] = bv; olp[r] = blp; }
        pc = bc; pv = bv;
    }
}

// One decision step t for every event (grid = events, 256 threads).  logits [rows, V1] are the step's finished logits (bias included).
// Per event: the alive slots' scores SCORE / ALIVE [rows], histories HTOK / HLP [rows, L], the result BTOK / BLP [events, L],
// BSCORE / BW [events] (words, -1: none yet).  t == 0 reads none of them (only slot 0 alive, score 0, no result).
// The carried state HS [rows, 3H] and C0..C2 [rows, H] (the decoder's h / c after step t) is permuted in place, and IT [rows] gets the
// tokens fed at step t+1.  A thread owns whole columns: it reads the column's parent values of all B slots before it writes any of them,
// so the in-place permutation needs no barrier and no LDS (a row of B = 16 slots at H = 512 is 196 KB).
template <int EPW>
__global__ __launch_bounds__(256) void beam_step_kernel(const float* __restrict__ logits, int V1, int B, int t, int L, int* __restrict__ IT,
                                                        float* __restrict__ SCORE, int* __restrict__ ALIVE, int* __restrict__ HTOK,
                                                        float* __restrict__ HLP, int* __restrict__ BTOK, float* __restrict__ BLP,
                                                        float* __restrict__ BSCORE, int* __restrict__ BW, float* __restrict__ HS,
                                                        float* __restrict__ C0, float* __restrict__ C1, float* __restrict__ C2, int H) {
    __shared__ float s_score[BEAM_MAX];
    __shared__ int s_alive[BEAM_MAX];
    __shared__ float cand_c[BEAM_MAX * BEAM_MAX], cand_lp[BEAM_MAX * BEAM_MAX];
    __shared__ int cand_v[BEAM_MAX * BEAM_MAX];
    __shared__ float win_c[BEAM_MAX], win_lp[BEAM_MAX];
    __shared__ int win_j[BEAM_MAX], win_v[BEAM_MAX];
    __shared__ int s_any, s_best, s_ident;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r0 = (long)e * B;
    if (tid < B) {
        s_alive[tid] = t == 0 ? (tid == 0) : ALIVE[r0 + tid];
        s_score[tid] = t == 0 ? 0.f : SCORE[r0 + tid];
        win_c[tid] = -INFINITY; win_j[tid] = 0; win_v[tid] = 0; win_lp[tid] = -INFINITY;          // (every rank is filled unless logits are NaN)
    }
    __syncthreads();
    if (tid == 0) {
        int any = 0;
        for (int j = 0; j < B; ++j) any |= s_alive[j];
        s_any = any;
    }
    __syncthreads();
    if (!s_any) return;          // (uniform) every hypothesis of this event has finished: its rows' outputs are ignored from here on
    // per alive slot: its row's top-B candidates (one wave per row)
    for (int j = wave; j < B; j += 4)
        if (s_alive[j]) beam_row_topb<EPW>(logits + (r0 + j) * V1, V1, B, s_score[j], lane, cand_c + j * B, cand_v + j * B, cand_lp + j * B);
    __syncthreads();
    // the B winners among the alive slots' B x B candidates: a candidate's rank is the number that rank before it (score, slot, token)
    if (tid < B * B) {
        const int j = tid / B;
        if (s_alive[j]) {
            const float c = cand_c[tid];
            const int v = cand_v[tid];
            int rank = 0;
            for (int q = 0; q < B * B; ++q) {
                const int jq = q / B;
                if (q == tid || !s_alive[jq]) continue;
                const float cq = cand_c[q];
                const int vq = cand_v[q];
                if (cq > c || (cq == c && (jq < j || (jq == j && vq < v)))) ++rank;
            }
            if (rank < B) { win_c[rank] = c; win_j[rank] = j; win_v[rank] = v; win_lp[rank] = cand_lp[tid]; }
        }
    }
    __syncthreads();
    // bookkeeping: the new slots, finished hypotheses offered to the result in slot order
    if (tid == 0) {
        float best = t == 0 ? -INFINITY : BSCORE[e];
        int bw = t == 0 ? -1 : BW[e], bk = -1, ident = 1;
        for (int k = 0; k < B; ++k) {
            const int v = win_v[k];
            const bool fin = v == 0 || t == L - 1;
            if (fin && (bw < 0 || win_c[k] > best)) { best = win_c[k]; bw = v == 0 ? t : L; bk = k; }
            SCORE[r0 + k] = win_c[k];
            ALIVE[r0 + k] = fin ? 0 : 1;
            IT[r0 + k] = (v >= 0 && v < V1) ? v : 0;
            ident &= win_j[k] == k;
        }
        BSCORE[e] = best;
        BW[e] = bw;
        s_best = bk;
        s_ident = ident;
    }
    __syncthreads();
    const int bk = s_best;
    // histories: positions < t take the parent's, position t the winner's token; the result copies the slot that replaced it
    for (int i = tid; i <= t; i += 256) {
        int tk[BEAM_MAX];
        float lp[BEAM_MAX];
        if (i < t) {
#pragma unroll
            for (int k = 0; k < BEAM_MAX; ++k)
                if (k < B) { const long src = (r0 + win_j[k]) * L + i; tk[k] = HTOK[src]; lp[k] = HLP[src]; }
        } else {
#pragma unroll
            for (int k = 0; k < BEAM_MAX; ++k)
                if (k < B) { tk[k] = win_v[k]; lp[k] = win_lp[k]; }
        }
#pragma unroll
        for (int k = 0; k < BEAM_MAX; ++k)
            if (k < B && (i == t || win_j[k] != k)) { HTOK[(r0 + k) * L + i] = tk[k]; HLP[(r0 + k) * L + i] = lp[k]; }
        if (bk >= 0) {
#pragma unroll
            for (int k = 0; k < BEAM_MAX; ++k)
                if (k == bk) { BTOK[(long)e * L + i] = tk[k]; BLP[(long)e * L + i] = lp[k]; }
        }
    }
    if (s_ident) return;
    // the carried decoder state: h of the three streams (HS row, 3H) and their cells (H each), column by column
    for (int q = tid; q < 6 * H; q += 256) {
        float* base;
        long ld;
        if (q < 3 * H) { base = HS + q; ld = 3 * H; }
        else {
            const int k3 = (q - 3 * H) / H;
            base = (k3 == 0 ? C0 : (k3 == 1 ? C1 : C2)) + (q - 3 * H - k3 * H);
            ld = H;
        }
        float val[BEAM_MAX];
#pragma unroll
        for (int k = 0; k < BEAM_MAX; ++k)
            if (k < B) val[k] = base[(r0 + win_j[k]) * ld];
#pragma unroll
        for (int k = 0; k < BEAM_MAX; ++k)
            if (k < B && win_j[k] != k) base[(r0 + k) * ld] = val[k];
    }
}

// seq [events, L] (the result's words, then zeros), seq_logp [events, L] (its log-probs up to and including <eos>, then zeros), score,
// words[e] and words[events] = the maximum over events: one workgroup
__global__ __launch_bounds__(256) void beam_finalize_kernel(const int* __restrict__ BTOK, const float* __restrict__ BLP,
                                                            const float* __restrict__ BSCORE, const int* __restrict__ BW, int E, int L,
                                                            long long* __restrict__ seq, float* __restrict__ seq_logp, float* __restrict__ score,
                                                            int* __restrict__ words) {
    __shared__ int red[4];
    int mx = 0;
    for (int e = threadIdx.x; e < E; e += 256) {
        const int w = max(0, min(L, BW[e]));
        for (int i = 0; i < L; ++i) {
            seq[(long)e * L + i] = i < w ? BTOK[(long)e * L + i] : 0;
            seq_logp[(long)e * L + i] = i <= w ? BLP[(long)e * L + i] : 0.f;
        }
        score[e] = BSCORE[e];
        words[e] = w;
        mx = max(mx, w);
    }
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) words[E] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// Multi-video batches (echr_decoder_beam_batch): video_words[v] = the largest words[e] among the events of video v, video_words[V] = the
// largest of all.  Workgroup v < V owns video v: vid (per ROW, B rows per event, non-decreasing) is searched for the video's run of events
// -- the first event whose row e*B has vid >= v up to the first with vid >= v+1 -- and the run's maximum is reduced in a fixed tree;
// workgroup V reduces every event.  Each output element has one writer and no workgroup reads another's, so the caller need not clear
// the vector and the result does not depend on the order the workgroups run in.  vid is only ever compared, never used as an index.
__device__ __forceinline__ int beam_first_event_at(const int* __restrict__ vid, int B, int E, int v) {          // first e in [0, E] with vid[e*B] >= v
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (vid[(long)mid * B] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__global__ __launch_bounds__(256) void beam_video_words_kernel(const int* __restrict__ words, const int* __restrict__ vid, int E, int B, int V,
                                                               int* __restrict__ video_words) {
    __shared__ int red[4];
    const int v = blockIdx.x;
    const int e0 = v < V ? beam_first_event_at(vid, B, E, v) : 0;
    const int e1 = v < V ? beam_first_event_at(vid, B, E, v + 1) : E;
    int mx = 0;
    for (int e = e0 + threadIdx.x; e < e1; e += 256) mx = max(mx, words[e]);
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) video_words[v] = max(max(red[0], red[1]), max(red[2], red[3]));
}

int beam_video_words(const int* words, const int* vid, int E, int B, int V, int* video_words, hipStream_t st) {
    hipLaunchKernelGGL(beam_video_words_kernel, dim3(V + 1), dim3(256), 0, st, words, vid, E, B, V, video_words);
    return check_launch("beam_video_words");
}

int beam_step(const float* logits, int V1, int E, int B, int t, int L, int* IT, const BeamState& bs, float* HS, float* C0, float* C1, float* C2,
              int H, hipStream_t st) {
#define ECHR_BEAM_LAUNCH(EPW)                                                                                                              \
    hipLaunchKernelGGL(beam_step_kernel<EPW>, dim3(E), dim3(256), 0, st, logits, V1, B, t, L, IT, bs.SCORE, bs.ALIVE, bs.HTOK, bs.HLP,   \
                       bs.BTOK, bs.BLP, bs.BSCORE, bs.BW, HS, C0, C1, C2, H)
    if (V1 <= 64 * 8) ECHR_BEAM_LAUNCH(8);
    else if (V1 <= 64 * 32) ECHR_BEAM_LAUNCH(32);
    else if (V1 <= 64 * 80) ECHR_BEAM_LAUNCH(80);          // ECHR / ActivityNet Captions widths (V1 = 5001)
    else ECHR_BEAM_LAUNCH(0);
#undef ECHR_BEAM_LAUNCH
    return check_launch("beam_step");
}

int beam_finalize(const BeamState& bs, int E, int L, long long* seq, float* seq_logp, float* score, int* words, hipStream_t st) {
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(1), dim3(256), 0, st, bs.BTOK, bs.BLP, bs.BSCORE, bs.BW, E, L, seq, seq_logp, score, words);
    return check_launch("beam_finalize");
}

}  // namespace echr
