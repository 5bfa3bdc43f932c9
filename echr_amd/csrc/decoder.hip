// Three-stream attention caption decoder on gfx950: the per-timestep kernels (frame-level additive
// attention score -> softmax -> context, LSTM-cell gate math with counter-based dropout) and the
// host-side sequence drivers that string them together with the MFMA projections of gemm.hip.
//
// Reference semantics: models/OldModel_NEW.py:98-137 (teacher-forced loop, get_logprobs_state),
// :376-401 (Attention), :801-823 (ThreeStream_Core), :139-187 (greedy sample).
//
// Data layout decisions:
//  * The clip context is never materialised as [N,A,D]: event n's slot a is row ev_start[n]+a of
//    c3d[Tv,D] (CaptionGenerator.py:147-151 builds a zero-padded copy instead).  ctx2att is applied ONCE
//    per forward to the Tv video rows (P_all[Tv,Ha]) instead of to N*A rows every timestep (:381).
//  * Padding slots are skipped: softmax over all A slots, x mask, / sum (:394-397) equals the softmax
//    over the valid slots (the padded terms cancel in the renormalisation).
//  * Time-major internal buffers [S, N, .]; only the log-prob output is written [N, S, V1].
//  * Because ss_prob == 0 (:36), the token/context halves of every W_ih product are batched over all
//    S*N rows before the recurrence; only W_hh.h and the attended-context columns are sequential.
#include <cstdlib>
#include <cstring>
#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

enum { SITE_TSRM = 0, SITE_H0 = 1, SITE_H1 = 2, SITE_H2 = 3, SITE_OUT = 4 };

static inline unsigned drop_thresh(float p) {
    if (p >= 1.f) return 0xFFFFFFFFu;
    double t = floor((double)p * 4294967296.0);
    return (unsigned)((unsigned long long)t & 0xFFFFFFFFull);
}
DropCfg make_drop(const echr_dropout* d, float p) {
    DropCfg c;
    c.k0 = (unsigned)(d ? (d->seed & 0xFFFFFFFFull) : 0);
    c.k1 = (unsigned)(d ? (d->seed >> 32) : 0);
    c.offset = d ? d->offset : 0;
    c.thresh = drop_thresh(p);
    c.scale = 1.0f / (1.0f - p);
    c.active = (d && d->training && p > 0.f) ? 1 : 0;
    return c;
}

// Tail stream: part B of the decoder backward (attention-parameter and token-embedding gradients: ~10 launches that nothing else in the
// backward pass depends on) can run on a second stream while autograd continues with the event encoder's / proposal encoder's
// backward on the caller's stream.  The caller joins with echr_stream_join (the Python side does it in an end-of-backward callback);
// every later library entry that takes a stream joins first as a safety net.
struct Tail { hipStream_t s = nullptr; hipEvent_t fork = nullptr, done = nullptr, fork2 = nullptr, done2 = nullptr, done3 = nullptr; bool ok = false, init = false, pending = false, pending3 = false; };
static Tail& tail() {
    static Tail t;
    if (!t.init) {
        t.init = true;
        bool good = hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.fork, echr::sync_event_flags()) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.done, echr::sync_event_flags()) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.fork2, echr::sync_event_flags()) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.done2, echr::sync_event_flags()) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.done3, echr::sync_event_flags()) == hipSuccess;
        t.ok = good;
    }
    return t;
}
// Several forks from one point of the caller's stream can share ONE recorded event (each hipEventRecord is a barrier packet the caller's
// next kernel queues behind: three of them in front of the event encoder's first kernel cost ~10 us).  fork_event(ev): the forks that
// follow wait for `ev` (already recorded on the caller's stream, nothing queued since) instead of recording their own; fork_event(nullptr) ends it.
static hipEvent_t& fork_event_slot() { static hipEvent_t e = nullptr; return e; }
void fork_event(hipEvent_t ev) { fork_event_slot() = ev; }
hipStream_t aux_fork(hipStream_t from) {
    Tail& t = tail();
    if (!t.ok) return nullptr;
    if (hipEvent_t fe = fork_event_slot()) return hipStreamWaitEvent(t.s, fe, 0) == hipSuccess ? t.s : nullptr;
    if (hipEventRecord(t.fork2, from) != hipSuccess || hipStreamWaitEvent(t.s, t.fork2, 0) != hipSuccess) return nullptr;
    return t.s;
}
int aux_join(hipStream_t to) {
    Tail& t = tail();
    if (hipEventRecord(t.done2, t.s) != hipSuccess || hipStreamWaitEvent(to, t.done2, 0) != hipSuccess) { set_error("stream join failed"); return -5; }
    return 0;
}
int join_tail(hipStream_t st) {
    Tail& t = tail();
    if (t.ok && t.pending) {
        t.pending = false;
        if (hipStreamWaitEvent(st, t.done, 0) != hipSuccess) { set_error("stream join failed"); return -5; }
    }
    if (t.ok && t.pending3) {          // the LSTM-layer gradient stage of an echr_decoder_bwd with async_tail = 2 (on the prepare stream)
        t.pending3 = false;
        if (hipStreamWaitEvent(st, t.done3, 0) != hipSuccess) { set_error("stream join failed"); return -5; }
    }
    return 0;
}

// Data-parallel hand-over points (echr_train_step_args.handover, echr_handover_wait): events recorded where a contiguous range of the
// gradient arena becomes final long before the backward pass ends -- the logit layer's gradients on the tail stream right behind their
// product, the three LSTM layers' gradients on the prepare stream behind the grouped weight-gradient product.  What persists here is what
// echr_handover_wait reads after the call: the events and which of them hold a point.  The request belongs to ONE backward pass and travels
// with it (DecCall.handover, copied into BwdPlan, where it is in force only when the events exist).
struct Handover { hipEvent_t ev[2] = {nullptr, nullptr}; bool valid[2] = {false, false}; bool init = false, ok = false; };
static Handover& handover() {
    static Handover h;
    if (!h.init) {
        h.init = true;
        // (system-scope release, unlike the library's internal edges: what waits for a hand-over point is a consumer OUTSIDE the library -- a
        // collective that peers read over xGMI, an SDMA copy -- and the events are only recorded when a hand-over was asked for)
        h.ok = hipEventCreateWithFlags(&h.ev[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&h.ev[1], hipEventDisableTiming) == hipSuccess;
        if (!h.ok) (void)hipGetLastError();
    }
    return h;
}
void handover_clear() { Handover& h = handover(); h.valid[0] = h.valid[1] = false; }
static int handover_mark(const DecCall& c, int which, hipStream_t on) {
    if (!c.handover) return 0;
    Handover& h = handover();
    if (hipEventRecord(h.ev[which], on) != hipSuccess) { set_error("decoder_bwd: hand-over event record failed"); return -5; }
    h.valid[which] = true;
    if (c.handover_cb) c.handover_cb(which, on, c.handover_user);          // (host callback: the caller queues its collective behind this point of `on`)
    return 0;
}
extern "C" int echr_handover_wait(int which, void* stream) {
    ECHR_REQUIRE(which == ECHR_HANDOVER_LOGIT || which == ECHR_HANDOVER_LSTM, "handover_wait: which must be 0 (logit layer) or 1 (LSTM layers)");
    Handover& h = handover();
    if (!h.ok || !h.valid[which]) return 1;
    if (hipStreamWaitEvent((hipStream_t)stream, h.ev[which], 0) != hipSuccess) { (void)hipGetLastError(); set_error("handover_wait: stream wait failed"); return -5; }
    return 0;
}

static int hop(hipStream_t from, hipEvent_t ev, hipStream_t to) {      // `to` continues after everything queued on `from`
    if (hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess) {
        set_error("stream fork/join failed");
        return -5;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// Frame-level attention.  All kernels index the video through (ev_start, ev_len); a workgroup = 4 waves, lanes across
// the feature axis in float4, one wave per group of slots.  Loads are branch-free (clamped addresses, masked
// contributions) and issued for ALL of a wave's slots before the first use, so each wave keeps 8-16 KB in flight.
// R  = float4 per lane per P_all row (ceil(Ha/256)), RD = float4 per lane per clip row (ceil(D/256)).
// ------------------------------------------------------------------------------------------------------
constexpr int MAXR = 4;   // Ha, D <= 1024

// score kernel: grid (N, ceil(A/32)): e[n,a] = alpha . tanh(P_all[start+a] + q[n]) + b_alpha.
// q[n,:] = b_h2a + sum of the split-K partial slabs of h1_prev . W_h^T (rec_gemm); block y==0 keeps it in QS for backward.
template <int R, int SLOTS>
__global__ __launch_bounds__(256) void att_score_kernel(const float* __restrict__ PALL, const float* __restrict__ QSL, int nslab,
                                                        long slab_stride, const float* __restrict__ b_q, float* __restrict__ QS,
                                                        const float* __restrict__ alpha, const float* __restrict__ b_alpha,
                                                        const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                        float* __restrict__ SC, int A, int Ha) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sq = sm;          // [Ha]
    float* sa = sm + Ha;     // [Ha]
    const int n = blockIdx.x, a0 = blockIdx.y * (4 * SLOTS);
    const int len = ev_len[n];
    if (a0 >= len) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row0 = ev_start[n];
    float4 p[SLOTS][R];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int a = min(a0 + wave * SLOTS + i, len - 1);
        const float* prow = PALL + (row0 + a) * Ha;
#pragma unroll
        for (int r = 0; r < R; ++r) p[i][r] = *reinterpret_cast<const float4*>(prow + min(lane * 4 + r * 256, Ha - 4));
    }
    for (int j = threadIdx.x; j < Ha; j += 256) {
        float q = b_q[j];
        for (int s = 0; s < nslab; ++s) q += QSL[s * slab_stride + (long)n * Ha + j];
        sq[j] = q; sa[j] = alpha[j];
        if (blockIdx.y == 0) QS[(long)n * Ha + j] = q;
    }
    __syncthreads();
    float4 q4[R], a4[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane * 4 + r * 256;
        const bool in = j < Ha;
        q4[r] = *reinterpret_cast<const float4*>(sq + min(j, Ha - 4));
        a4[r] = *reinterpret_cast<const float4*>(sa + min(j, Ha - 4));
        if (!in) a4[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float ba = b_alpha[0];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            acc += a4[r].x * fast_tanh(p[i][r].x + q4[r].x) + a4[r].y * fast_tanh(p[i][r].y + q4[r].y) +
                   a4[r].z * fast_tanh(p[i][r].z + q4[r].z) + a4[r].w * fast_tanh(p[i][r].w + q4[r].w);
        }
        acc = wave_sum(acc);
        const int a = a0 + wave * SLOTS + i;
        if (lane == 0 && a < len) SC[(long)n * A + a] = acc + ba;
    }
}

// context kernel: grid (N, ceil(D/128)); softmax over the event's valid slots, then ctx[n, d-chunk] =
// sum_a w_a * c3d[start+a, d-chunk]; 32 float4 lanes across the chunk x 8 row groups, LDS combine.
__global__ __launch_bounds__(256) void att_context_kernel(const float* __restrict__ C3D, const float* __restrict__ SC,
                                                          const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                          float* __restrict__ WT, float* __restrict__ ATT, int A, int D) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int A32 = (A + 31) & ~31;
    float* w = sm;                       // [A32] (zero beyond len)
    float* red = sm + A32;               // [8][128]
    __shared__ float r4[4];
    const int n = blockIdx.x, d0 = blockIdx.y * 128;
    const int len = ev_len[n];
    const long row0 = ev_start[n];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float m = -INFINITY;
    for (int a = threadIdx.x; a < len; a += 256) m = fmaxf(m, SC[(long)n * A + a]);
    m = wave_max(m);
    if (lane == 0) r4[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(r4[0], r4[1]), fmaxf(r4[2], r4[3]));
    __syncthreads();
    float s = 0.f;
    for (int a = threadIdx.x; a < A32; a += 256) {
        const float e = a < len ? __expf(SC[(long)n * A + a] - m) : 0.f;
        w[a] = e; s += e;
    }
    s = wave_sum(s);
    if (lane == 0) r4[wave] = s;
    __syncthreads();
    const float inv = 1.0f / (r4[0] + r4[1] + r4[2] + r4[3]);
    for (int a = threadIdx.x; a < A32; a += 256) {
        const float wa = w[a] * inv;
        w[a] = wa;
        if (blockIdx.y == 0 && a < A) WT[(long)n * A + a] = wa;
    }
    __syncthreads();
    const int dl = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int d = min(d0 + dl * 4, D - 4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ab = 0; ab < len; ab += 32) {          // 4 rows per thread in flight
        float4 c[4];
        float wa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int a = ab + rg + 8 * u;
            wa[u] = w[a];                             // zero past the event's end
            c[u] = *reinterpret_cast<const float4*>(C3D + (row0 + min(a, len - 1)) * D + d);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { acc.x += wa[u] * c[u].x; acc.y += wa[u] * c[u].y; acc.z += wa[u] * c[u].z; acc.w += wa[u] * c[u].w; }
    }
    *reinterpret_cast<float4*>(red + rg * 128 + dl * 4) = acc;
    __syncthreads();
    if (threadIdx.x < 128) {
        const int dd = d0 + threadIdx.x;
        if (dd < D) {
            float t = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) t += red[g * 128 + threadIdx.x];
            ATT[(long)n * D + dd] = t;
        }
    }
}

// backward for one timestep.  grid (N, ceil(A/32)).
//   dscore_a = w_a * (clip_a . dATT - ATT . dATT);  dq += sum_a dscore_a * alpha * (1 - tanh^2(P_a + q))
// dATT arrives as split-K slabs (rec_gemm).  DSC keeps dscore for the post-recurrence pass that accumulates d P_all and
// d alpha over all timesteps (that pass recomputes tanh instead of updating an [N,A,Ha] accumulator every step).
template <int R, int RD, int SLOTS>
__global__ __launch_bounds__(256) void att_bwd_kernel(const float* __restrict__ PALL, const float* __restrict__ C3D,
                                                      const float* __restrict__ Q, const float* __restrict__ alpha,
                                                      const float* __restrict__ WT, const float* __restrict__ ATT,
                                                      const float* __restrict__ DAS, int nslab, long slab_stride,
                                                      const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                      float* __restrict__ DSC, float* __restrict__ DQ, int A, int Ha, int D, long dq_slab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sq = sm;                 // [Ha]
    float* sa = sq + Ha;            // [Ha]
    const int D4 = (D + 3) & ~3;
    float* sd = sa + Ha;            // [D4] dATT row
    float* red = sd + D4;           // [4][Ha]
    __shared__ float r4[4];
    const int n = blockIdx.x, a0 = blockIdx.y * (4 * SLOTS);
    const int len = ev_len[n];
    if (a0 >= len) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row0 = ev_start[n];
    float4 p[SLOTS][R], c[SLOTS][RD];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int a = min(a0 + wave * SLOTS + i, len - 1);
        const float* crow = C3D + (row0 + a) * D;
        const float* prow = PALL + (row0 + a) * Ha;
#pragma unroll
        for (int r = 0; r < RD; ++r) c[i][r] = *reinterpret_cast<const float4*>(crow + min(lane * 4 + r * 256, D - 4));
#pragma unroll
        for (int r = 0; r < R; ++r) p[i][r] = *reinterpret_cast<const float4*>(prow + min(lane * 4 + r * 256, Ha - 4));
    }
    float s0 = 0.f;
    for (int j = threadIdx.x; j < Ha; j += 256) { sq[j] = Q[(long)n * Ha + j]; sa[j] = alpha[j]; }
    for (int j = threadIdx.x; j < D4; j += 256) {
        float dv = 0.f;
        if (j < D)
            for (int s = 0; s < nslab; ++s) dv += DAS[s * slab_stride + (long)n * D + j];
        sd[j] = dv;
        if (j < D) s0 += dv * ATT[(long)n * D + j];
    }
    s0 = wave_sum(s0);
    if (lane == 0) r4[wave] = s0;
    __syncthreads();
    s0 = r4[0] + r4[1] + r4[2] + r4[3];
    float dsc[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        float dw = 0.f;
#pragma unroll
        for (int r = 0; r < RD; ++r) {
            const int j = lane * 4 + r * 256;
            if (j < D) {
                const float4 g = *reinterpret_cast<const float4*>(sd + j);
                dw += c[i][r].x * g.x + c[i][r].y * g.y + c[i][r].z * g.z + c[i][r].w * g.w;
            }
        }
        dw = wave_sum(dw);
        const int a = a0 + wave * SLOTS + i;
        dsc[i] = a < len ? WT[(long)n * A + min(a, A - 1)] * (dw - s0) : 0.f;
        if (lane == 0 && a < len) DSC[(long)n * A + a] = dsc[i];
    }
    float4 dq[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        dq[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int j = min(lane * 4 + r * 256, Ha - 4);
        const float4 q4 = *reinterpret_cast<const float4*>(sq + j);
        const float4 a4 = *reinterpret_cast<const float4*>(sa + j);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            float t;
            t = fast_tanh(p[i][r].x + q4.x); dq[r].x += dsc[i] * a4.x * (1.f - t * t);
            t = fast_tanh(p[i][r].y + q4.y); dq[r].y += dsc[i] * a4.y * (1.f - t * t);
            t = fast_tanh(p[i][r].z + q4.z); dq[r].z += dsc[i] * a4.z * (1.f - t * t);
            t = fast_tanh(p[i][r].w + q4.w); dq[r].w += dsc[i] * a4.w * (1.f - t * t);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane * 4 + r * 256;
        if (j < Ha) *reinterpret_cast<float4*>(red + wave * Ha + j) = dq[r];
    }
    __syncthreads();
    // dq_slab != 0 (fixed-order mode): DQ is a stack of per-chunk slabs, summed in chunk order by dq_fold_kernel
    if (dq_slab) {
        for (int j = threadIdx.x; j < Ha; j += 256)
            DQ[(long)blockIdx.y * dq_slab + (long)n * Ha + j] = red[j] + red[Ha + j] + red[2 * Ha + j] + red[3 * Ha + j];
        return;
    }
    for (int j = threadIdx.x; j < Ha; j += 256)
        atomicAdd(&DQ[(long)n * Ha + j], red[j] + red[Ha + j] + red[2 * Ha + j] + red[3 * Ha + j]);
}
// fixed-order mode: d q[n, :] += the slabs of the event's ceil(len / chunk) attention workgroups, in chunk order
__global__ __launch_bounds__(256) void dq_fold_kernel(const float* __restrict__ slabs, long slab_stride, const int* __restrict__ ev_len,
                                                      float* __restrict__ DQ, int N, int Ha, int chunk) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * Ha) return;
    const int n = (int)(idx / Ha);
    const int ny = (ev_len[n] + chunk - 1) / chunk;
    float s = 0.f;
    for (int y = 0; y < ny; ++y) s += slabs[(long)y * slab_stride + idx];
    DQ[idx] += s;
}

// Post-recurrence pass: d P_all[row,:] += sum_t dsc_t * alpha * (1 - tanh^2(P_row + q_t)),
//                       d alpha      += sum_{t,n,a} dsc_t * tanh(P_row + q_t),  d b_alpha += sum dsc.
// grid (N, ceil(A/8)): 4 waves x 2 slots; q_t[n,:] for a tile of TT timesteps is staged in LDS (4 workgroups per CU).
constexpr int TT = 10;
constexpr int PSLOTS = 2;
constexpr int ALPHA_REP = 32;       // replicas of d alpha / d b_alpha that att_post accumulates into
template <int R>
__global__ __launch_bounds__(256) void att_post_kernel(const float* __restrict__ PALL, const float* __restrict__ QS,
                                                       const float* __restrict__ alpha, const float* __restrict__ DSC,
                                                       const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                       float* __restrict__ DPALL, float* __restrict__ g_alpha,
                                                       float* __restrict__ g_balpha, int S, int N, int A, int Ha, int disjoint, int alpha_rows, unsigned* __restrict__ dom) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sqt = sm;                   // [TT][Ha]
    float* sds = sqt + TT * Ha;        // [TT][8] dscore tile
    float* red = sds + TT * 8;         // [4][Ha]
    __shared__ float wsum[4];
    const int n = blockIdx.x, a0 = blockIdx.y * 8;
    const int len = ev_len[n];
    if (a0 >= len) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row0 = ev_start[n];
    float4 p[PSLOTS][R], a4[R], dal[R];
    // 1 - tanh^2(p + q) = 4 r (1 - r), tanh(p + q) = 1 - 2 r with r = 1 / (e^{2p} e^{2q} + 1): e^{2p} once per row, e^{2q} once per staged q
    // element -- one fma + rcp per (slot, feature, timestep) instead of an exp + rcp (arguments clamped to +-43: never inf * 0)
    // The form is tanh(p + q) only while |p| <= 43 and |q| <= 43: an argument outside is reported through `dom` (the host-mapped flag block,
    // echr_internal.h DOMAIN_WORD_P / DOMAIN_WORD_Q: largest magnitude seen; -EDOM at the next library call), never silently clamped
    float pmax = 0.f, qmax = 0.f;
#pragma unroll
    for (int i = 0; i < PSLOTS; ++i) {
        const int a = min(a0 + wave * PSLOTS + i, len - 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 pv = *reinterpret_cast<const float4*>(PALL + (row0 + a) * Ha + min(lane * 4 + r * 256, Ha - 4));
            pmax = fmaxf(fmaxf(pmax, fmaxf(fabsf(pv.x), fabsf(pv.y))), fmaxf(fabsf(pv.z), fabsf(pv.w)));
            p[i][r] = make_float4(__expf(2.f * fminf(fmaxf(pv.x, -43.f), 43.f)), __expf(2.f * fminf(fmaxf(pv.y, -43.f), 43.f)),
                                  __expf(2.f * fminf(fmaxf(pv.z, -43.f), 43.f)), __expf(2.f * fminf(fmaxf(pv.w, -43.f), 43.f)));
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane * 4 + r * 256;
        a4[r] = j < Ha ? *reinterpret_cast<const float4*>(alpha + j) : make_float4(0.f, 0.f, 0.f, 0.f);
        dal[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 dp[PSLOTS][R];
#pragma unroll
    for (int i = 0; i < PSLOTS; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) dp[i][r] = make_float4(0.f, 0.f, 0.f, 0.f);
    float dsum = 0.f;
    for (int t0 = 0; t0 < S; t0 += TT) {
        const int nt = min(TT, S - t0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < nt * 8; idx += 256) {
            const int tt = idx >> 3, i = idx & 7;
            sds[idx] = (a0 + i < len) ? DSC[((long)(t0 + tt) * N + n) * A + a0 + i] : 0.f;
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < nt * (Ha >> 2); idx += 256) {
            const int tt = idx / (Ha >> 2), j4 = idx % (Ha >> 2);
            const float4 qv = *reinterpret_cast<const float4*>(QS + ((long)(t0 + tt) * N + n) * Ha + 4 * j4);
            // (domain check on the rows that are consumed only: a position behind a caption's end has d score = 0 for every slot, is skipped below,
            // and its q row may never have been written)
            const float4 d0 = *reinterpret_cast<const float4*>(sds + tt * 8), d1 = *reinterpret_cast<const float4*>(sds + tt * 8 + 4);
            if (d0.x != 0.f || d0.y != 0.f || d0.z != 0.f || d0.w != 0.f || d1.x != 0.f || d1.y != 0.f || d1.z != 0.f || d1.w != 0.f)
                qmax = fmaxf(fmaxf(qmax, fmaxf(fabsf(qv.x), fabsf(qv.y))), fmaxf(fabsf(qv.z), fabsf(qv.w)));
            *reinterpret_cast<float4*>(sqt + tt * Ha + 4 * j4) =
                make_float4(__expf(2.f * fminf(fmaxf(qv.x, -43.f), 43.f)), __expf(2.f * fminf(fmaxf(qv.y, -43.f), 43.f)),
                            __expf(2.f * fminf(fmaxf(qv.z, -43.f), 43.f)), __expf(2.f * fminf(fmaxf(qv.w, -43.f), 43.f)));
        }
        __syncthreads();
        for (int tt = 0; tt < nt; ++tt) {
#pragma unroll
            for (int i = 0; i < PSLOTS; ++i) {
                const float dsc = sds[tt * 8 + wave * PSLOTS + i];
                // d score is exactly zero at every position behind a caption's end (about 40% of all (t, n) at S = 20) and contributes nothing:
                // the slot is wave-uniform, so the skip costs one scalar branch
                if ((__builtin_amdgcn_readfirstlane(__float_as_int(dsc)) << 1) == 0) continue;
                dsum += dsc;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 q4 = *reinterpret_cast<const float4*>(sqt + tt * Ha + min(lane * 4 + r * 256, Ha - 4));
                    float rr;          // dp accumulates dsc * r (1 - r) (x 4 at the end); dal accumulates dsc * r (tanh = 1 - 2 r, fixed up at the end)
                    rr = __builtin_amdgcn_rcpf(fmaf(p[i][r].x, q4.x, 1.f)); dp[i][r].x = fmaf(dsc, rr - rr * rr, dp[i][r].x); dal[r].x = fmaf(dsc, rr, dal[r].x);
                    rr = __builtin_amdgcn_rcpf(fmaf(p[i][r].y, q4.y, 1.f)); dp[i][r].y = fmaf(dsc, rr - rr * rr, dp[i][r].y); dal[r].y = fmaf(dsc, rr, dal[r].y);
                    rr = __builtin_amdgcn_rcpf(fmaf(p[i][r].z, q4.z, 1.f)); dp[i][r].z = fmaf(dsc, rr - rr * rr, dp[i][r].z); dal[r].z = fmaf(dsc, rr, dal[r].z);
                    rr = __builtin_amdgcn_rcpf(fmaf(p[i][r].w, q4.w, 1.f)); dp[i][r].w = fmaf(dsc, rr - rr * rr, dp[i][r].w); dal[r].w = fmaf(dsc, rr, dal[r].w);
                }
            }
        }
    }
    if (dom) {
        if (pmax > 43.f) __hip_atomic_store(dom + DOMAIN_WORD_P, __float_as_uint(pmax), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (qmax > 43.f) __hip_atomic_store(dom + DOMAIN_WORD_Q, __float_as_uint(qmax), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int i = 0; i < PSLOTS; ++i) {
        const int a = a0 + wave * PSLOTS + i;
        if (a < len) {
            float* drow = DPALL + (row0 + a) * Ha;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = lane * 4 + r * 256;
                if (j < Ha) {
                    const float4 dv = make_float4(4.f * dp[i][r].x * a4[r].x, 4.f * dp[i][r].y * a4[r].y, 4.f * dp[i][r].z * a4[r].z, 4.f * dp[i][r].w * a4[r].w);
                    if (disjoint == 2) {      // fixed-order mode: DPALL is an [N][A][Ha] slab stack, folded per video row in event order (dpall_fold_kernel)
                        *reinterpret_cast<float4*>(DPALL + ((long)n * A + a) * Ha + j) = dv;
                    } else if (disjoint) {      // the row belongs to this event alone: plain 16-byte store
                        *reinterpret_cast<float4*>(drow + j) = dv;
                    } else {
                        atomicAdd(drow + j + 0, dv.x);
                        atomicAdd(drow + j + 1, dv.y);
                        atomicAdd(drow + j + 2, dv.z);
                        atomicAdd(drow + j + 3, dv.w);
                    }
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane * 4 + r * 256;
        // sum dsc * tanh = sum dsc * (1 - 2 r) = dsum - 2 * (sum dsc * r)
        if (j < Ha) *reinterpret_cast<float4*>(red + wave * Ha + j) = make_float4(dsum - 2.f * dal[r].x, dsum - 2.f * dal[r].y, dsum - 2.f * dal[r].z, dsum - 2.f * dal[r].w);
    }
    __syncthreads();
    // ALPHA_REP replicas of the two parameter gradients, summed by a column-sum launch afterwards: the N * ceil(A/8) workgroups used to
    // add into ONE [Ha] vector (1024 adders per address on 16 cache lines: those atomics, not the arithmetic, were the kernel's 66 us)
    if (alpha_rows) {          // fixed-order mode: one (pre-zeroed) row per workgroup, summed in row order by the column-sum launch behind
        const long rep = blockIdx.x + (long)blockIdx.y * gridDim.x;
        for (int j = threadIdx.x; j < Ha; j += 256) g_alpha[rep * Ha + j] = red[j] + red[Ha + j] + red[2 * Ha + j] + red[3 * Ha + j];
        // d b_alpha: every lane of a wave holds the same dsum over the wave's two slots; the four waves' values in wave order
        if (lane == 0) wsum[wave] = dsum;
        __syncthreads();
        if (threadIdx.x == 0) g_balpha[rep] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        return;
    }
    const int rep = (int)((blockIdx.x + blockIdx.y * gridDim.x) % ALPHA_REP);
    for (int j = threadIdx.x; j < Ha; j += 256)
        atomicAdd(&g_alpha[(long)rep * Ha + j], red[j] + red[Ha + j] + red[2 * Ha + j] + red[3 * Ha + j]);
    if (lane == 0 && dsum != 0.f) atomicAdd(g_balpha + rep, dsum);
}
// fixed-order mode: d P_all[row, :] += the slab rows of the events that cover video row `row`, in event order
__global__ __launch_bounds__(256) void dpall_fold_kernel(const float* __restrict__ slab, const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                         float* __restrict__ DPALL, int N, int A, int Ha) {
    const int row = blockIdx.x;
    for (int j = threadIdx.x; j < Ha; j += 256) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) {
            const int a = row - ev_start[n];
            if (a >= 0 && a < ev_len[n]) s += slab[((long)n * A + a) * Ha + j];
        }
        DPALL[(long)row * Ha + j] += s;
    }
}

// ---- launch helpers (dispatch on the per-lane row widths) ------------------------------------------------
struct AttDims { int N, A, Ha, D; };

static int att_slots() {     // slots per wave (2, 4 or 8): tuning knob, default chosen from measurements on the c3 workload
    const int v = config().att_slots;
    return (v == 2 || v == 4 || v == 8) ? v : 2;
}

static int launch_att_score(const AttDims& d, const float* PALL, const float* QSL, int nslab, long slab_stride, const float* b_q,
                            float* QS, const float* alpha, const float* b_alpha, const int* ev_start, const int* ev_len, float* SC,
                            hipStream_t st) {
    const int SL = att_slots();
    const dim3 grid(d.N, (d.A + 4 * SL - 1) / (4 * SL)), blk(256);
    const size_t sm = 2 * d.Ha * sizeof(float);
    const int R = (d.Ha + 255) / 256;
#define ECHR_CASE(RR, SS) if (R == RR && SL == SS) { hipLaunchKernelGGL((att_score_kernel<RR, SS>), grid, blk, sm, st, PALL, QSL, nslab, slab_stride, b_q, QS, alpha, b_alpha, ev_start, ev_len, SC, d.A, d.Ha); return check_launch("att_score"); }
    ECHR_CASE(1, 2) ECHR_CASE(2, 2) ECHR_CASE(3, 2) ECHR_CASE(4, 2)
    ECHR_CASE(1, 4) ECHR_CASE(2, 4) ECHR_CASE(3, 4) ECHR_CASE(4, 4)
    ECHR_CASE(1, 8) ECHR_CASE(2, 8) ECHR_CASE(3, 8) ECHR_CASE(4, 8)
#undef ECHR_CASE
    set_error("att_score: Ha too large");
    return -22;
}

static int launch_att_bwd(const AttDims& d, const float* PALL, const float* C3D, const float* Q, const float* alpha, const float* WT,
                          const float* ATT, const float* DAS, int nslab, long slab_stride, const int* ev_start, const int* ev_len,
                          float* DSC, float* DQ, hipStream_t st) {
    const int SL = att_slots();
    const dim3 grid(d.N, (d.A + 4 * SL - 1) / (4 * SL)), blk(256);
    const size_t sm = (6 * d.Ha + ((d.D + 3) & ~3)) * sizeof(float);
    const int R = (d.Ha + 255) / 256, RD = (d.D + 255) / 256;
    // fixed-order mode: per-chunk slabs of d q + a fold launch in chunk order instead of atomic adds
    const long dq_slab = det_mode() ? (long)d.N * d.Ha : 0L;
    float* dq_out = DQ;
    if (dq_slab) {
        dq_out = det_scratch(DET_DQ, (size_t)grid.y * dq_slab);
        if (!dq_out) return -12;
    }
    auto fold = [&]() -> int {
        if (!dq_slab) return check_launch("att_bwd");
        if (int rc = check_launch("att_bwd")) return rc;
        hipLaunchKernelGGL(dq_fold_kernel, dim3((unsigned)((dq_slab + 255) / 256)), dim3(256), 0, st, dq_out, dq_slab, ev_len, DQ, d.N, d.Ha, 4 * SL);
        return check_launch("dq_fold");
    };
#define ECHR_CASE3(RR, RRD, SS) if (R == RR && RD == RRD && SL == SS) { hipLaunchKernelGGL((att_bwd_kernel<RR, RRD, SS>), grid, blk, sm, st, PALL, C3D, Q, alpha, WT, ATT, DAS, nslab, slab_stride, ev_start, ev_len, DSC, dq_out, d.A, d.Ha, d.D, dq_slab); return fold(); }
#define ECHR_CASE(RR, RRD) ECHR_CASE3(RR, RRD, 2) ECHR_CASE3(RR, RRD, 4) ECHR_CASE3(RR, RRD, 8)
    ECHR_CASE(1, 1) ECHR_CASE(1, 2) ECHR_CASE(2, 1) ECHR_CASE(2, 2) ECHR_CASE(2, 3) ECHR_CASE(2, 4) ECHR_CASE(3, 2) ECHR_CASE(4, 2)
    ECHR_CASE(1, 3) ECHR_CASE(1, 4) ECHR_CASE(3, 1) ECHR_CASE(3, 3) ECHR_CASE(3, 4) ECHR_CASE(4, 1) ECHR_CASE(4, 3) ECHR_CASE(4, 4)
#undef ECHR_CASE
#undef ECHR_CASE3
    set_error("att_bwd: Ha or D too large");
    return -22;
}

static int launch_att_post(const AttDims& d, const float* PALL, const float* QS, const float* alpha, const float* DSC, const int* ev_start,
                           const int* ev_len, float* DPALL, float* g_alpha, float* g_balpha, int S, int disjoint, hipStream_t st, int alpha_rows = 0) {
    if (config().diag_skip & 4) return 0;
    const dim3 grid(d.N, (d.A + 7) / 8), blk(256);
    const size_t sm = ((size_t)TT * d.Ha + TT * 8 + 4 * d.Ha) * sizeof(float);
    switch ((d.Ha + 255) / 256) {
#define ECHR_CASE(R) case R: hipLaunchKernelGGL((att_post_kernel<R>), grid, blk, sm, st, PALL, QS, alpha, DSC, ev_start, ev_len, DPALL, g_alpha, g_balpha, S, d.N, d.A, d.Ha, disjoint, alpha_rows, persist_host_flag()); break;
        ECHR_CASE(1) ECHR_CASE(2) ECHR_CASE(3) ECHR_CASE(4)
#undef ECHR_CASE
        default: set_error("att_post: Ha too large"); return -22;
    }
    return check_launch("att_post");
}

// ------------------------------------------------------------------------------------------------------
// Grouped skinny NT GEMM for the recurrence: P[ks] = A[M, kslice] . B[Nout, kslice]^T, M = events (<= a few
// hundred), several independent problems ("jobs") per launch, K split over workgroups.  Partial sums go to
// per-slice slabs that the CONSUMER kernel adds up (LSTM gate math / attention) -- no atomics, no extra
// reduction launch, bitwise reproducible.
//   grid (ceil(Nout/64), ksplit, jobs * ceil(M/64)); 256 threads = 2x2 waves of 32x32 MFMA tiles.
//   A and B k-slices are staged once into LDS with full-row coalesced float4 loads ([64][128+4] floats each,
//   conflict-free ds_read_b128 fragment reads); 2 workgroups per CU overlap one's loads with the other's MFMAs.
//   Lane l feeds MFMA j of an 8-wide k chunk with element j of its float4 (k = 8c + 4(l>>5) + j): A and B use
//   the same k pairing, so the products are exact fp32 sums over the slice.
// ------------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int RK = 128;          // k-slice staged per workgroup
constexpr int RQ = RK / 4, RLP = 64 * RQ / 256;      // float4 per row, staging float4 per thread and operand
constexpr int RLD = RK + 4;          // LDS row stride (floats): 16-byte aligned rows, conflict-free b128 reads
constexpr int MAXJOBS = 8;

struct RecJob {
    const float* A; long lda; int K;
    const float* B; long ldb; int Nout;
    float* P; long slab_stride; long ldp;
    int atomic;      // 1: all k-slices add atomically into ONE pre-zeroed slab (for outputs that many workgroups re-read,
                     //    where summing slabs in every consumer would multiply the traffic); order-dependent last bits
    const int* rowidx;   // optional row gather: row m of the A operand is A[rowidx[m]] (the sampler's embedding rows by token id)
};
struct RecArgs { RecJob job[MAXJOBS]; int njobs; int M; int kloop = 0; };

__global__ __launch_bounds__(256, 2) void rec_gemm_kernel(RecArgs args) {
    constexpr int NT = 256;
    __shared__ __attribute__((aligned(16))) float smem[2 * 64 * RLD];      // 67,584 B: A tile | B tile
    float* As = smem;
    float* Bs = smem + 64 * RLD;
    const int jz = blockIdx.z % args.njobs, rb = blockIdx.z / args.njobs;
    const RecJob J = args.job[jz];
    const int n0 = blockIdx.x * 64, m0 = rb * 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // args.kloop (grid.y = 1): this workgroup walks ALL k slices of its tile in order and updates the output once (no host path sets it: the
    // fixed-order mode runs the slab form of rec_gemm)
    const int ks0 = args.kloop ? 0 : (int)blockIdx.y, ks1 = args.kloop ? (J.K + RK - 1) / RK : ks0 + 1;
    if (n0 >= J.Nout || ks0 * RK >= J.K) return;
    for (int ks = ks0; ks < ks1; ++ks) {
    const int k0 = ks * RK;
    const int k1 = min(J.K, k0 + RK);
    if (ks > ks0) __syncthreads();          // the previous slice's fragment reads are done
    // branch-free staging: every lane loads from a clamped (always valid) address and zeroes what lies outside the
    // problem, so all global loads of a thread are in flight together before the first LDS write
    constexpr int LP = RLP;
    float4 va[LP], vb[LP];
#pragma unroll
    for (int p = 0; p < LP; ++p) {
        const int f = tid + p * NT;
        const int row = f / RQ, kq = (f % RQ) * 4;
        const int kk = min(k0 + kq, J.K - 4);
        const int ra = min(m0 + row, args.M - 1), rbn = min(n0 + row, J.Nout - 1);
        va[p] = *reinterpret_cast<const float4*>(J.A + (long)(J.rowidx ? J.rowidx[ra] : ra) * J.lda + kk);
        vb[p] = *reinterpret_cast<const float4*>(J.B + (long)rbn * J.ldb + kk);
    }
#pragma unroll
    for (int p = 0; p < LP; ++p) {
        const int f = tid + p * NT;
        const int row = f / RQ, kq = (f % RQ) * 4;
        const bool kin = (k0 + kq) < k1;
        const float ma = (kin && (m0 + row) < args.M) ? 1.f : 0.f;
        const float mb = (kin && (n0 + row) < J.Nout) ? 1.f : 0.f;
        float4 a = va[p], b = vb[p];
        a.x *= ma; a.y *= ma; a.z *= ma; a.w *= ma;
        b.x *= mb; b.y *= mb; b.z *= mb; b.w *= mb;
        *reinterpret_cast<float4*>(&As[row * RLD + kq]) = a;
        *reinterpret_cast<float4*>(&Bs[row * RLD + kq]) = b;
    }
    __syncthreads();
    const float* ap = &As[(wm + l31) * RLD + 4 * h];
    const float* bp = &Bs[(wn + l31) * RLD + 4 * h];
    // the whole slice is always multiplied (tails are zero-filled): a fixed trip count lets the compiler
    // hoist the LDS fragment reads ahead of the MFMA chain
#pragma unroll
    for (int c = 0; c < RK / 8; ++c) {
        const float4 a4 = *reinterpret_cast<const float4*>(ap + 8 * c);
        const float4 b4 = *reinterpret_cast<const float4*>(bp + 8 * c);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
    }
    }
    float* P = J.P + (J.atomic ? 0L : (long)blockIdx.y * J.slab_stride);
    const int col = n0 + wn + l31;
    if (col < J.Nout) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row < args.M) {
                if (J.atomic && args.kloop) P[(long)row * J.ldp + col] += acc[r];          // the tile's only writer in this launch
                else if (J.atomic) atomicAdd(&P[(long)row * J.ldp + col], acc[r]);
                else P[(long)row * J.ldp + col] = acc[r];
            }
        }
    }
}

static inline int ksplit_of(int K) { return (K + RK - 1) / RK; }

// fixed-order mode: P[j][row, col] += the job's k-slice slabs, in slice order (one thread per output element of every job)
struct RecFold { float* P[MAXJOBS]; const float* slab[MAXJOBS]; long ldp[MAXJOBS]; long start[MAXJOBS + 1]; int Nout[MAXJOBS]; int nslab[MAXJOBS]; int njobs; int M; };
__global__ __launch_bounds__(256) void rec_fold_kernel(RecFold f) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= f.start[f.njobs]) return;
    int j = 0;
    while (j + 1 < f.njobs && idx >= f.start[j + 1]) ++j;
    const long e = idx - f.start[j];
    const int row = (int)(e / f.Nout[j]), col = (int)(e % f.Nout[j]);
    const long sl = (long)f.M * f.Nout[j];
    float s = 0.f;
    for (int k = 0; k < f.nslab[j]; ++k) s += f.slab[j][(long)k * sl + e];
    f.P[j][(long)row * f.ldp[j] + col] += s;
}

static int rec_gemm(const RecArgs& a, hipStream_t st) {
    int maxn = 0, maxk = 0;
    double fl = 0, by = 0;
    for (int j = 0; j < a.njobs; ++j) {
        const RecJob& J = a.job[j];
        ECHR_REQUIRE(J.K % 4 == 0 && J.lda % 4 == 0 && J.ldb % 4 == 0 && ((uintptr_t)J.A % 16 == 0) && ((uintptr_t)J.B % 16 == 0),
                     "rec_gemm: operands must be 16-byte aligned with K, lda, ldb multiples of 4 (job %d)", j);
        maxn = max(maxn, (J.Nout + 63) / 64);
        maxk = max(maxk, ksplit_of(J.K));
        fl += 2.0 * a.M * J.Nout * J.K;
        by += 4.0 * ((double)a.M * J.K + (double)J.Nout * J.K + (double)a.M * J.Nout * ksplit_of(J.K));
    }
    ProfScope prof(PROF_LSTM, fl, by, st);
    bool any_atomic = false;
    for (int j = 0; j < a.njobs; ++j) any_atomic = any_atomic || a.job[j].atomic;
    if (det_mode() && any_atomic) {
        // fixed-order mode for the jobs that add into shared accumulators (slab jobs are not mixed in)
        for (int j = 0; j < a.njobs; ++j) ECHR_REQUIRE(a.job[j].atomic, "rec_gemm: fixed-order mode cannot mix slab and accumulator jobs");
        for (int j = 1; j < a.njobs; ++j) for (int i = 0; i < j; ++i) ECHR_REQUIRE(a.job[i].P != a.job[j].P, "rec_gemm: fixed-order mode needs distinct outputs per launch");
        // every k slice writes its own slab (the launch keeps its k parallelism), then ONE fold launch adds a job's slabs to its accumulator
        // in slice order: 6 + 4 us instead of one 28-us workgroup per tile walking all sixteen slices
        RecArgs b = a;
        RecFold f;
        f.njobs = a.njobs; f.M = a.M;
        long need = 0;
        for (int j = 0; j < a.njobs; ++j) need += (long)ksplit_of(a.job[j].K) * a.M * a.job[j].Nout;
        float* scr = det_scratch(DET_REC, (size_t)need);
        if (!scr) return -12;
        long off = 0, cells = 0;
        for (int j = 0; j < a.njobs; ++j) {
            const long sl = (long)a.M * a.job[j].Nout;
            f.P[j] = a.job[j].P; f.ldp[j] = a.job[j].ldp; f.Nout[j] = a.job[j].Nout; f.nslab[j] = ksplit_of(a.job[j].K); f.slab[j] = scr + off; f.start[j] = cells;
            b.job[j].P = scr + off; b.job[j].slab_stride = sl; b.job[j].ldp = a.job[j].Nout; b.job[j].atomic = 0;
            off += sl * f.nslab[j];
            cells += sl;
        }
        f.start[a.njobs] = cells;
        hipLaunchKernelGGL(rec_gemm_kernel, dim3(maxn, maxk, a.njobs * ((a.M + 63) / 64)), dim3(256), 0, st, b);
        if (int rc = check_launch("rec_gemm")) return rc;
        hipLaunchKernelGGL(rec_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, f);
        return check_launch("rec_fold");
    }
    hipLaunchKernelGGL(rec_gemm_kernel, dim3(maxn, maxk, a.njobs * ((a.M + 63) / 64)), dim3(256), 0, st, a);
    return check_launch("rec_gemm");
}

// ------------------------------------------------------------------------------------------------------
// LSTM cell gate math for the three streams of one timestep (nn.LSTMCell order i,f,g,o).
// Pre-activation = input-side part (GATES, batched GEMM before the recurrence) + the recurrent split-K slabs.
// GATES is overwritten with the activations (saved for backward).  h is dropped once for the recurrence/state
// (OldModel_NEW.py:810,814,818) and once more for the late-fusion input (:136).
// ------------------------------------------------------------------------------------------------------
struct LstmPtrs {
    float* gates[3];          // [N,4H] slice of timestep t
    const float* slab[3];     // recurrent partial sums: slab[k] + s*slab_stride, s < nslab[k]
    int nslab[3];
    long slab_stride;
    const float* c_prev[3];
    float* c_new[3];
    int kmap[3];              // blockIdx.y -> stream index (lets a launch cover a subset of the streams)
    // optional (sampler): time-invariant part of the pre-activation read from base[k] + (n % bmod[k]) * 4H (+ base2[k], a [4H] vector) instead
    // of from `gates` -- the token-side products then arrive as slabs like the recurrent ones, and no per-step input-gate GEMM runs
    const float* base[3]; const float* base2[3]; int bmod[3];
};

__global__ __launch_bounds__(256) void lstm_pointwise_fwd_kernel(LstmPtrs P, float* __restrict__ h_out, float* __restrict__ outd,
                                                                 int N, int H, int t, DropCfg dh, DropCfg dout) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * H) return;
    const int k = P.kmap[blockIdx.y];
    const int n = idx / H, j = idx % H;
    float* g = P.gates[k] + (long)n * 4 * H;
    float pi, pf, pg, po;
    if (P.base[k]) {
        const float* bq = P.base[k] + (long)(n % P.bmod[k]) * 4 * H;
        pi = bq[j]; pf = bq[H + j]; pg = bq[2 * H + j]; po = bq[3 * H + j];
        if (P.base2[k]) { const float* b2 = P.base2[k]; pi += b2[j]; pf += b2[H + j]; pg += b2[2 * H + j]; po += b2[3 * H + j]; }
    } else { pi = g[j]; pf = g[H + j]; pg = g[2 * H + j]; po = g[3 * H + j]; }
    const float* sl = P.slab[k] + (long)n * 4 * H;
    for (int s = 0; s < P.nslab[k]; ++s) {
        const float* q = sl + s * P.slab_stride;
        pi += q[j]; pf += q[H + j]; pg += q[2 * H + j]; po += q[3 * H + j];
    }
    const float gi = fast_sigmoid(pi), gf = fast_sigmoid(pf), gg = tanhf(pg), go = fast_sigmoid(po);
    const float c = gf * P.c_prev[k][idx] + gi * gg;
    g[j] = gi; g[H + j] = gf; g[2 * H + j] = gg; g[3 * H + j] = go;
    P.c_new[k][idx] = c;
    const float h = go * tanhf(c) * drop_mult(dh, (unsigned)idx, (unsigned)t, (unsigned)(SITE_H0 + k));
    const long o = (long)n * 3 * H + k * H + j;
    h_out[o] = h;
    outd[o] = h * drop_mult(dout, (unsigned)o, (unsigned)t, SITE_OUT);
}

struct LstmBwdPtrs {
    const float* gates[3];    // activations of timestep t
    const float* c_prev[3];
    const float* c_new[3];
    float* dgates[3];         // [N,4H] slice of timestep t
    const float* dh_slab[3];  // partial sums of d h(t) from step t+1: [N,H] slabs
    float* dh_acc[3];         // or (accumulate mode) ONE [N,H] buffer per stream that step t+1 added into atomically: read, then re-zeroed
    int nslab[3];
    long slab_stride;
    int kmap[3];
};

// dh = dOUTD * m_out + sum of the recurrent slabs written while processing step t+1;  dC carries c-gradients.
__global__ __launch_bounds__(256) void lstm_pointwise_bwd_kernel(LstmBwdPtrs P, const float* __restrict__ doutd, float* __restrict__ dc,
                                                                 int N, int H, int t, DropCfg dh, DropCfg dout) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * H) return;
    const int k = P.kmap[blockIdx.y];
    const int n = idx / H, j = idx % H;
    const long o = (long)n * 3 * H + k * H + j;
    float dhv = doutd[o] * drop_mult(dout, (unsigned)o, (unsigned)t, SITE_OUT);
    if (P.dh_acc[k]) { dhv += P.dh_acc[k][idx]; P.dh_acc[k][idx] = 0.f; }
    for (int s = 0; s < P.nslab[k]; ++s) dhv += P.dh_slab[k][s * P.slab_stride + idx];
    dhv *= drop_mult(dh, (unsigned)idx, (unsigned)t, (unsigned)(SITE_H0 + k));
    const float* g = P.gates[k] + (long)n * 4 * H;
    const float gi = g[j], gf = g[H + j], gg = g[2 * H + j], go = g[3 * H + j];
    const float tc = tanhf(P.c_new[k][idx]);
    const float dcv = dhv * go * (1.f - tc * tc) + dc[o];
    float* dg = P.dgates[k] + (long)n * 4 * H;
    dg[j] = dcv * gg * gi * (1.f - gi);
    dg[H + j] = dcv * P.c_prev[k][idx] * gf * (1.f - gf);
    dg[2 * H + j] = dcv * gi * (1.f - gg * gg);
    dg[3 * H + j] = dhv * tc * go * (1.f - go);
    dc[o] = dcv * gf;
}

// ------------------------------------------------------------------------------------------------------
// workspace carving
// ------------------------------------------------------------------------------------------------------
static inline long rup(long x, long a) { return (x + a - 1) / a * a; }

// Multi-video batches: the caller's scratch echr_batch_ext.ws = VIDB [N, 4H] (scene part of stream 2's gates per EVENT) | VIDV [V, 4H] (per
// video) | DGSEG [V, 4H] (d gates2 summed over time and over the events of a video).  The workspaces below are those of a single video.
struct BatchWs { float *VIDB, *VIDV, *DGSEG; long total; };
static BatchWs carve_batch(long N, long V, long H, float* base) {
    BatchWs w;
    long off = 0;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += rup(n, 64); return p; };
    w.VIDB = take(N * 4 * H); w.VIDV = take(V * 4 * H); w.DGSEG = take(V * 4 * H);
    w.total = off;
    return w;
}
struct DecWs {
    float *XT, *GATES[3], *CS[3], *HS, *OUTD, *PALL, *QS, *SC, *WT, *ATT, *EVB0, *VIDB;
    float *QSL, *GSL[3];         // split-K slabs of the current timestep (q and the three gate blocks)
    float *QACC;                 // [S,N,Ha] atomic accumulation target of q (teacher-forced path)
    float *PK_C3D, *PK_WC, *PK_WIH[3], *PK_WL, *PK_XT, *PK_OUTD;     // h2-packed GEMM operands of the forward pass
    float *XWS;                  // exchange buffers + counters of the persistent recurrence kernel (csrc/persist.hip)
    float *PK_WLT;               // W_logit^T packed for the backward's d OUTD product (echr_dec_args.train: packed with the forward operands)
    int nq, ng[3];
    long total;
    // the scene part of stream 2's gate pre-activations: one [4H] vector (VIDB, pitch 0) or, for a multi-video batch (bx, nullptr otherwise), one
    // row per event in the caller's batch scratch (pitch 4H), consumed like stream 0's per-event EVB0; scene_rows: see DecCall
    const echr_batch_ext* bx; float* scene; long scene_ld; bool scene_rows;
};
static DecWs carve_ws(const echr_dec_args* a, float* base, const echr_batch_ext* bx = nullptr, bool scene_rows = false) {
    DecWs w;
    long off = 0;
    const long N = a->N, S = a->S, H = a->H;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += rup(n, 64); return p; };
    w.XT = take(S * N * a->E);
    for (int k = 0; k < 3; ++k) w.GATES[k] = take(S * N * 4 * H);
    for (int k = 0; k < 3; ++k) w.CS[k] = take((S + 1) * N * H);
    w.HS = take((S + 1) * N * 3 * H);
    w.OUTD = take(S * N * 3 * H);
    w.PALL = take((long)a->Tv * a->Ha);
    w.QS = take(S * N * a->Ha);
    w.SC = take(S * N * a->A);
    w.WT = take(S * N * a->A);
    w.ATT = take(S * N * a->D);
    w.EVB0 = take(N * 4 * H);
    w.VIDB = take(4 * H);
    w.nq = ksplit_of(a->H);
    w.QSL = take((long)w.nq * N * a->Ha);
    w.QACC = take(S * N * a->Ha);
    // slabs per stream: W_hh . h, (stream 1: W_ih1[:, E:] . ctx), and -- sampler only -- the token-side product W_ih[:, :E] . embed(token)
    w.ng[0] = w.ng[2] = ksplit_of(a->H) + ksplit_of(a->E);
    w.ng[1] = ksplit_of(a->H) + ksplit_of(a->D) + ksplit_of(a->E);
    for (int k = 0; k < 3; ++k) w.GSL[k] = take((long)w.ng[k] * N * 4 * H);
    w.PK_C3D = take(h2_floats(a->Tv, a->D));
    w.PK_WC = take(h2_floats(a->Ha, a->D));
    for (int k = 0; k < 3; ++k) w.PK_WIH[k] = take(h2_floats(4 * a->H, a->E));
    w.PK_WL = take(h2_floats(a->V1, 3 * a->H));
    w.PK_XT = take(h2_floats((int)(S * N), a->E));
    w.PK_OUTD = take(h2_floats((int)(S * N), 3 * a->H));
    w.XWS = take(persist_fwd_ws_floats((int)S));
    w.PK_WLT = take(h2_floats(3 * a->H, a->V1));
    w.total = off;
    w.bx = bx; w.scene_rows = bx && scene_rows;
    w.scene = bx ? carve_batch(N, bx->n_videos, H, bx->ws).VIDB : w.VIDB;
    w.scene_ld = bx ? 4 * H : 0;
    return w;
}

struct DecWsBwd {
    float *DLG, *DOUT, *DG[3], *DC, *DSC, *DQ, *DPALL, *DGSUM[3], *DGCOL[3], *DXT, *MSUM, *ROWL;
    float *WT_HH[3], *WT_ATT, *WT_H2A;      // transposed weights: the backward recurrence runs as NT products too
    float *WLT, *DLGT, *OUTDT;               // W_logit^T [3H, ldg], DLG^T [V1, snp], OUTD^T [3H, snp]: NT operands for the split GEMM
    // h2-packed operands of the backward GEMMs (suffix T: packed from the transposed view, i.e. contraction over rows of the source)
    float *PK_DLGT, *PK_OUTDT, *PK_DLG, *PK_WLT, *PK_DGT[3], *PK_DG[3], *PK_HT[3], *PK_XTT, *PK_ATTT, *PK_DQT, *PK_WIHT[3], *PK_DPT, *PK_C3DT;
    long snp;
    float *DHACC[3], *DASL;                  // atomic accumulation targets: d h(t-1) per stream [N,H]; DASL: d ATT [S,N,D]
    float *GAREP, *GBREP;                    // replicated attention-vector gradients (att_post_kernel)
    float *XWSB;                             // exchange buffers + counters of the persistent reverse recurrence (csrc/persist.hip)
    long ldg, total, zero_floats;
};
static DecWsBwd carve_ws_bwd(const echr_dec_args* a, float* base) {
    DecWsBwd w;
    long off = 0;
    const long N = a->N, S = a->S, H = a->H;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += rup(n, 64); return p; };
    w.ldg = rup(a->V1, 4);
    w.DLG = take(S * N * w.ldg);
    w.DOUT = take(S * N * 3 * H);
    for (int k = 0; k < 3; ++k) w.DG[k] = take(S * N * 4 * H);
    w.DSC = take(S * N * a->A);
    // one contiguous zero-initialised region: DC | DGCOL | DHACC | DQ | DASL | DPALL (a single fill per backward)
    w.DC = take(N * 3 * H);
    for (int k = 0; k < 3; ++k) w.DGCOL[k] = take(4 * H);
    for (int k = 0; k < 3; ++k) w.DHACC[k] = take(N * H);
    w.DQ = take(S * N * a->Ha);
    w.DASL = take(S * N * a->D);
    w.GAREP = take((long)ALPHA_REP * a->Ha);      // att_post's replicated d alpha, then [ALPHA_REP] d b_alpha
    w.GBREP = take(ALPHA_REP);
    w.DPALL = take((long)a->Tv * a->Ha);
    w.zero_floats = (w.DPALL - w.DC) + rup((long)a->Tv * a->Ha, 64);
    for (int k = 0; k < 3; ++k) w.DGSUM[k] = take(N * 4 * H);
    w.DXT = take(S * N * a->E);
    w.MSUM = take(64);
    w.ROWL = take(S * N);
    for (int k = 0; k < 3; ++k) w.WT_HH[k] = take(H * 4 * H);
    w.WT_ATT = take((long)a->D * 4 * H);
    w.WT_H2A = take(H * (long)a->Ha);
    w.snp = rup(S * N, 4);
    w.WLT = take(3 * H * w.ldg);
    w.DLGT = take((long)a->V1 * w.snp);
    w.OUTDT = take(3 * H * w.snp);
    const int SN = (int)(S * N), H4 = 4 * a->H;
    w.PK_DLGT = take(h2_floats(a->V1, SN)); w.PK_OUTDT = take(h2_floats(3 * a->H, SN));
    w.PK_DLG = take(h2_floats(SN, a->V1)); w.PK_WLT = take(h2_floats(3 * a->H, a->V1));
    for (int k = 0; k < 3; ++k) {
        w.PK_DGT[k] = take(h2_floats(H4, SN)); w.PK_DG[k] = take(h2_floats(SN, H4));
        w.PK_HT[k] = take(h2_floats(a->H, SN)); w.PK_WIHT[k] = take(h2_floats(a->E, H4));
    }
    w.PK_XTT = take(h2_floats(a->E, SN)); w.PK_ATTT = take(h2_floats(a->D, SN)); w.PK_DQT = take(h2_floats(a->Ha, SN));
    w.PK_DPT = take(h2_floats(a->Ha, a->Tv)); w.PK_C3DT = take(h2_floats(a->D, a->Tv));
    w.XWSB = take(persist_bwd_ws_floats((int)S));
    w.total = off;
    return w;
}

static int check_dims(const echr_dec_args* a, const char* who) {
    ECHR_REQUIRE(a, "%s: null args", who);
    ECHR_REQUIRE(a->N > 0 && a->A > 0 && a->Tv > 0 && a->S >= 0, "%s: bad N/A/Tv/S", who);
    ECHR_REQUIRE(a->D % 4 == 0 && a->Ha % 4 == 0 && a->Ha <= 256 * MAXR && a->D <= 256 * MAXR && a->D >= 4 && a->Ha >= 4,
                 "%s: need D%%4==0, Ha%%4==0, 4 <= D,Ha <= %d (D=%d Ha=%d)", who, 256 * MAXR, a->D, a->Ha);
    ECHR_REQUIRE(a->H > 0 && a->E > 0 && a->De > 0 && a->Dv > 0 && a->V1 > 1, "%s: bad widths", who);
    ECHR_REQUIRE(a->H % 4 == 0 && a->E % 4 == 0, "%s: need H%%4==0 and E%%4==0 (H=%d E=%d)", who, a->H, a->E);
    return 0;
}
int check_dims_public(const echr_dec_args* a, const char* who) { return check_dims(a, who); }
// what the clip-row gradient (clipctx.hip) reads from a finished echr_decoder_bwd / echr_decoder_fwd on the same workspaces
void decoder_bwd_views(const echr_dec_args* a, const echr_dec_grads* g, const float** dg1, const float** dpall) {
    const DecWsBwd b = carve_ws_bwd(a, g->ws_bwd);
    *dg1 = b.DG[1];
    *dpall = b.DPALL;
}
const float* decoder_fwd_wt(const echr_dec_args* a) { return carve_ws(a, a->ws).WT; }

#define RC(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

static RecJob mkjob(const float* A, long lda, int K, const float* B, long ldb, int Nout, float* P, long slab_stride, long ldp,
                    int atomic = 0) {
    RecJob j; j.A = A; j.lda = lda; j.K = K; j.B = B; j.ldb = ldb; j.Nout = Nout; j.P = P; j.slab_stride = slab_stride; j.ldp = ldp;
    j.atomic = atomic; j.rowidx = nullptr;
    return j;
}

// P_all = c3d . W_c^T + b_c over the Tv video rows; EVB0 = event . W_ih0[:,E:]^T + b_ih0 + b_hh0;
// VIDB = W_ih2[:,E:] . video + b_ih2 + b_hh2   (all time-invariant)
// parts: 1 = everything that does not read the event context (operand packs, P_all, VIDB), 2 = EVB0
// wl: optional second stream for the two packed images of W_logit (the logits product's operand and, in training, its transpose for d OUTD): they
// are 60 % of the pack launch's bytes and nothing in front of the forward recurrence reads them, so echr_decoder_fwd_prepare puts them on the
// CALLER's stream -- whose later logits / d OUTD products follow in stream order -- instead of at the head of the prepare chain
static int precompute_static(const echr_dec_args* a, const DecWs& w, hipStream_t st, bool teacher_forced, bool evb0_zeroed = false, int parts = 3,
                             hipStream_t wl = nullptr) {
    const int H = a->H, E = a->E;
    echr_gemm_desc d;
    if (!(parts & 1)) goto event_part;
    if (config().gemm_h2) {
        // every time-invariant GEMM operand of the forward pass is packed by one launch
        H2PackJob pj[7] = {pack_rows(a->c3d, a->D, a->Tv, a->D, w.PK_C3D), pack_rows(a->w_c2a, a->D, a->Ha, a->D, w.PK_WC),
                           pack_rows(a->w_logit, 3 * H, a->V1, 3 * H, w.PK_WL), pack_rows(a->w_ih[0], E + a->De, 4 * H, E, w.PK_WIH[0]),
                           pack_rows(a->w_ih[1], E + a->D, 4 * H, E, w.PK_WIH[1]), pack_rows(a->w_ih[2], E + a->Dv, 4 * H, E, w.PK_WIH[2]),
                           pack_cols(a->w_logit, 3 * H, 3 * H, a->V1, w.PK_WLT)};      // (train: the backward's operand, off its critical path)
        if (wl && teacher_forced) {
            H2PackJob pa[5] = {pj[0], pj[1], pj[3], pj[4], pj[5]}, pb[2] = {pj[2], pj[6]};
            RC(h2_pack_multi(pb, a->train ? 2 : 1, wl));
            RC(h2_pack_multi(pa, 5, st));
        } else
        RC(h2_pack_multi(pj, teacher_forced ? (a->train ? 7 : 6) : 2, st));      // the sampler's per-step products stay on the skinny-GEMM path
        d = desc_h2(w.PK_C3D, w.PK_WC, w.PALL, a->Ha, a->Tv, a->Ha, a->D);
    } else {
        d = desc_nt(a->c3d, a->D, a->w_c2a, a->D, w.PALL, a->Ha, a->Tv, a->Ha, a->D);
        d.split_k = -1; d.algo = ECHR_GEMM_BF16X3;
    }
    d.bias = a->b_c2a;
    RC(gemm(d, st));
    if (const echr_batch_ext* bx = w.bx) {
        // multi-video batch: one scene vector per video -> VIDV [V, 4H] (one fixed-order k loop per tile), gathered by vid into the per-event
        // VIDB [N, 4H] that the gate products / kernels consume exactly as they consume stream 0's per-event EVB0
        const BatchWs bw = carve_batch(a->N, bx->n_videos, H, bx->ws);
        if (w.scene_rows) {          // every video's vector exactly as its own call forms it (DecCall.scene_rows)
            RC(rows_matvec(bx->video, a->Dv, a->w_ih[2] + E, E + a->Dv, a->b_ih[2], a->b_hh[2], bw.VIDV, 4 * H, bx->n_videos, 4 * H, a->Dv, st));
        } else {
            d = desc_nt(bx->video, a->Dv, a->w_ih[2] + E, E + a->Dv, bw.VIDV, 4 * H, bx->n_videos, 4 * H, a->Dv);
            d.bias = a->b_ih[2]; d.bias2 = a->b_hh[2]; d.split_k = 1;
            RC(gemm(d, st));
        }
        RC(embed_gather(bw.VIDV, bx->vid, bw.VIDB, a->N, 4 * H, bx->n_videos, st));
    } else
    RC(row_matvec(a->video, a->w_ih[2] + E, E + a->Dv, a->b_ih[2], a->b_hh[2], w.VIDB, 4 * H, a->Dv, st));      // (M = 1: no GEMM launch)
event_part:
    if (parts & 2) {
        d = desc_nt(a->event, a->De, a->w_ih[0] + E, E + a->De, w.EVB0, 4 * H, a->N, 4 * H, a->De);
        d.bias = a->b_ih[0]; d.bias2 = a->b_hh[0]; d.split_k = -1;
        if (evb0_zeroed) d.beta = 1.f;            // accumulate into the caller's zeros: no fill launch
        RC(gemm(d, st));
    }
    return 0;
}

// G[t][n][:] += B[n][:] for every timestep (the event-context part of stream 0's gate pre-activations, added after the fact when the
// token-side products were computed ahead of the event encoder)
__global__ __launch_bounds__(256) void add_bcast_rows_kernel(float* __restrict__ G, const float* __restrict__ B, long rows, long per_step, int cols4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols4) return;
    const long r = i / cols4, c = i % cols4;
    float4 g = reinterpret_cast<float4*>(G)[i];
    const float4 b = reinterpret_cast<const float4*>(B)[(r % per_step) * cols4 + c];
    g.x += b.x; g.y += b.y; g.z += b.z; g.w += b.w;
    reinterpret_cast<float4*>(G)[i] = g;
}

// non-zero initial state (echr_dec_args.h0 [N, 3H]): h(-1) = HS[0] (same layout) and c_k(-1) = CS[k][0] = h0[:, kH:(k+1)H]
__global__ __launch_bounds__(256) void init_state_copy_kernel(const float* __restrict__ h0, float* __restrict__ HS0, float* __restrict__ C0, float* __restrict__ C1,
                                                              float* __restrict__ C2, int N, int H) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * 3 * H) return;
    const int n = (int)(i / (3 * H)), c = (int)(i % (3 * H)), k = c / H, j = c % H;
    const float v = h0[i];
    HS0[i] = v;
    (k == 0 ? C0 : (k == 1 ? C1 : C2))[(long)n * H + j] = v;
}
// d loss / d h0 [N, 3H] = d h(-1) (what step 0's recurrent products left in the d h accumulators) + d c(-1) (the carried cell gradient)
__global__ __launch_bounds__(256) void init_state_grad_kernel(const float* __restrict__ DH0, const float* __restrict__ DH1, const float* __restrict__ DH2,
                                                              const float* __restrict__ DC, float* __restrict__ g_h0, int N, int H) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * 3 * H) return;
    const int n = (int)(i / (3 * H)), c = (int)(i % (3 * H)), k = c / H, j = c % H;
    g_h0[i] = (k == 0 ? DH0 : (k == 1 ? DH1 : DH2))[(long)n * H + j] + DC[i];
}
static int init_state_copy(const echr_dec_args* a, const DecWs& w, hipStream_t st) {
    const long n = (long)a->N * 3 * a->H;
    hipLaunchKernelGGL(init_state_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a->h0, w.HS, w.CS[0], w.CS[1], w.CS[2], a->N, a->H);
    return check_launch("init_state_copy");
}

// one decoder timestep given the input-side gate pre-activations already in GATES[k][t]
//   launch 1: q and the three W_hh . h(t-1) products (all depend only on h(t-1))      -> slabs
//   launch 2,3: attention scores, softmax + context
//   launch 4: attended-context columns of stream 1's W_ih                              -> slabs
//   launch 5: gate math for the three streams (adds the slabs)
static int step_fwd(const echr_dec_args* a, const DecWs& w, int t, const DropCfg& dh, const DropCfg& dout, hipStream_t st, bool q_atomic = false,
                    const int* tok = nullptr) {
    const int N = a->N, H = a->H, Ha = a->Ha, A = a->A, D = a->D, E = a->E;
    const float* hprev = w.HS + (long)t * N * 3 * H;          // [N,3H] dropped h of step t-1 (zeros at t=0)
    const long gs = (long)N * 4 * H, qs = (long)N * Ha;
    const int nh = ksplit_of(H);
    RecArgs ra;
    ra.M = N; ra.njobs = 0;
    // q is re-read by every attention workgroup of an event: accumulate it atomically into one buffer (training) instead of
    // letting each of them sum the k-slice slabs; the sampler keeps the slab form (bitwise reproducible decoding)
    float* qacc = q_atomic ? w.QACC + (long)t * N * Ha : w.QSL;
    ra.job[ra.njobs++] = mkjob(hprev + H, 3 * H, H, a->w_h2a, H, Ha, qacc, qs, Ha, q_atomic ? 1 : 0);
    // training path: the recurrent products add atomically into GATES[k][t], which already holds the input-side pre-activations,
    // so the gate kernel reads one value per gate instead of summing 4..8 slabs (the sampler keeps the reproducible slab form)
    const bool gacc = q_atomic;
    for (int k = 0; k < 3; ++k)
        ra.job[ra.njobs++] = gacc ? mkjob(hprev + k * H, 3 * H, H, a->w_hh[k], H, 4 * H, w.GATES[k] + (long)t * gs, gs, 4 * H, 1)
                                  : mkjob(hprev + k * H, 3 * H, H, a->w_hh[k], H, 4 * H, w.GSL[k], gs, 4 * H);
    const int ne = ksplit_of(E), nd = ksplit_of(D);
    if (tok) {
        // sampler, few events: the token-side products W_ih_k[:, :E] . embed(token) ride in the same launch (A rows gathered from the embedding
        // table by token id); their k-slices are slabs behind the stream's other slabs, summed by the gate kernel in a fixed order
        for (int k = 0; k < 3; ++k) {
            const int cin_k = E + (k == 0 ? a->De : (k == 1 ? D : a->Dv));
            RecJob j = mkjob(a->embed, E, E, a->w_ih[k], cin_k, 4 * H, w.GSL[k] + (long)(nh + (k == 1 ? nd : 0)) * gs, gs, 4 * H);
            j.rowidx = tok;
            ra.job[ra.njobs++] = j;
        }
    }
    RC(rec_gemm(ra, st));
    float* q = w.QS + (long)t * N * Ha;
    float* sc = w.SC + (long)t * N * A;
    float* wt = w.WT + (long)t * N * A;
    float* att = w.ATT + (long)t * N * D;
    {
    // algorithmic bytes of one attention step: p_att rows + clip rows + scores/weights/context
    const double rows = (double)N * A;
    ProfScope prof(PROF_ATT_FWD, 2.0 * rows * (Ha + D) , 4.0 * (rows * (Ha + D + 2) + (double)N * (Ha + D)), st);
    const AttDims ad{N, A, Ha, D};
    RC(launch_att_score(ad, w.PALL, qacc, q_atomic ? 1 : w.nq, qs, a->b_h2a, q, a->w_alpha, a->b_alpha, a->ev_start, a->ev_len, sc, st));
    hipLaunchKernelGGL(att_context_kernel, dim3(N, (D + 127) / 128), dim3(256), (((A + 31) & ~31) + 8 * 128) * sizeof(float), st, a->c3d, sc,
                       a->ev_start, a->ev_len, wt, att, A, D);
    RC(check_launch("att_context"));
    }
    ra.njobs = 1;
    ra.job[0] = gacc ? mkjob(att, D, D, a->w_ih[1] + E, E + D, 4 * H, w.GATES[1] + (long)t * gs, gs, 4 * H, 1)
                     : mkjob(att, D, D, a->w_ih[1] + E, E + D, 4 * H, w.GSL[1] + nh * gs, gs, 4 * H);
    RC(rec_gemm(ra, st));
    LstmPtrs P;
    for (int k = 0; k < 3; ++k) {
        P.gates[k] = w.GATES[k] + (long)t * N * 4 * H;
        P.slab[k] = w.GSL[k];
        P.nslab[k] = gacc ? 0 : (nh + (k == 1 ? nd : 0) + (tok ? ne : 0));
        P.base[k] = nullptr; P.base2[k] = nullptr; P.bmod[k] = 1;
        if (tok) {
            if (k == 0) { P.base[k] = w.EVB0; P.bmod[k] = N; }
            else if (k == 1) { P.base[k] = a->b_ih[1]; P.base2[k] = a->b_hh[1]; }
            else { P.base[k] = w.scene; if (w.bx) P.bmod[k] = N; }          // (multi-video batch: per-event scene part)
        }
        P.c_prev[k] = w.CS[k] + (long)t * N * H;
        P.c_new[k] = w.CS[k] + (long)(t + 1) * N * H;
        P.kmap[k] = k;
    }
    P.slab_stride = gs;
    hipLaunchKernelGGL(lstm_pointwise_fwd_kernel, dim3((N * H + 255) / 256, 3), dim3(256), 0, st, P,
                       w.HS + (long)(t + 1) * N * 3 * H, w.OUTD + (long)t * N * 3 * H, N, H, t, dh, dout);
    return check_launch("lstm_pointwise_fwd");
}

// input-side gate pre-activations for `rows` = nt*N token rows starting at timestep t0
static int input_gates(const echr_dec_args* a, const DecWs& w, const float* xt, int t0, int nt, hipStream_t st, bool no_evb0 = false, bool force_h2 = false,
                       bool xt_packed = false) {
    const int N = a->N, H = a->H, E = a->E;
    const int rows = nt * N;
    const int cin[3] = {E + a->De, E + a->D, E + a->Dv};
    echr_gemm_desc d[3];
    // the teacher-forced call (all S*N token rows at once), or a sampler step over many events (force_h2: PK_WIH packed by the caller)
    const bool h2 = config().gemm_h2 && ((xt == w.XT && t0 == 0 && nt == a->S) || force_h2);
    if (h2 && !xt_packed) {
        H2PackJob pj = pack_rows(xt, E, rows, E, w.PK_XT);
        RC(h2_pack_multi(&pj, 1, st));
    }
    for (int k = 0; k < 3; ++k) {
        float* g = w.GATES[k] + (long)t0 * N * 4 * H;
        d[k] = h2 ? desc_h2(w.PK_XT, w.PK_WIH[k], g, 4 * H, rows, 4 * H, E) : desc_nt(xt, E, a->w_ih[k], cin[k], g, 4 * H, rows, 4 * H, E);
        d[k].add_mod = N; d[k].ld_add = 4 * H;
        if (k == 0) { if (!no_evb0) d[k].addend = w.EVB0; }
        else if (k == 1) { d[k].bias = a->b_ih[1]; d[k].bias2 = a->b_hh[1]; }
        else if (w.bx) d[k].addend = w.scene;          // multi-video batch: the scene part is per event, like EVB0
        else d[k].bias = w.VIDB;
        d[k].split_k = force_h2 ? 1 : -1;          // sampler: one fixed-order k loop per tile (bitwise reproducible)
    }
    return gemm_grouped(d, 3, st);       // the three streams' token-side products in one launch
}

// ---- the frame-level attention launches as the one-stream decoder (sat.hip) calls them: q arrives as ONE finished [N, Ha] product
// (without its bias), d ATT as one [N, D] buffer ----
int att_score_launch(const AttShape& s, const float* PALL, const float* Q1, const float* b_q, float* QS, const float* alpha, const float* b_alpha,
                     const int* ev_start, const int* ev_len, float* SC, hipStream_t st) {
    const AttDims ad{s.N, s.A, s.Ha, s.D};
    return launch_att_score(ad, PALL, Q1, 1, (long)s.N * s.Ha, b_q, QS, alpha, b_alpha, ev_start, ev_len, SC, st);
}
int att_context_launch(const AttShape& s, const float* C3D, const float* SC, const int* ev_start, const int* ev_len, float* WT, float* ATT, hipStream_t st) {
    hipLaunchKernelGGL(att_context_kernel, dim3(s.N, (s.D + 127) / 128), dim3(256), (((s.A + 31) & ~31) + 8 * 128) * sizeof(float), st, C3D, SC, ev_start, ev_len,
                       WT, ATT, s.A, s.D);
    return check_launch("att_context");
}
int att_bwd_launch(const AttShape& s, const float* PALL, const float* C3D, const float* Q, const float* alpha, const float* WT, const float* ATT,
                   const float* DATT, const int* ev_start, const int* ev_len, float* DSC, float* DQ, hipStream_t st) {
    const AttDims ad{s.N, s.A, s.Ha, s.D};
    return launch_att_bwd(ad, PALL, C3D, Q, alpha, WT, ATT, DATT, 1, (long)s.N * s.D, ev_start, ev_len, DSC, DQ, st);
}
// d P_all (into the zero-filled DPALL [Tv, Ha]) and d alpha / d b_alpha (ADDED to g_alpha / g_balpha) over all S steps; GAREP / GBREP: the
// zero-filled replica scratch [ALPHA_REP, Ha] / [ALPHA_REP] of the atomic form (att_post_replicas())
int att_post_replicas() { return ALPHA_REP; }
// att_post in fixed-order form (deterministic mode), no atomics: one d alpha / d b_alpha row per workgroup (*ga [*nblk, Ha], *gb [*nblk] in det_scratch;
// their column sums stay with the caller) and, for events that share video rows, one d P_all slab row per (event, position), folded into DPALL in order
static int att_post_fixed_order(const AttDims& ad, int Tv, int S, int rows_disjoint, const float* PALL, const float* QS, const float* alpha, const float* DSC,
                                const int* ev_start, const int* ev_len, float* DPALL, float** ga, float** gb, int* nblk, hipStream_t st) {
    const long nb = (long)ad.N * ((ad.A + 7) / 8);
    *ga = det_scratch(DET_ALPHA, (size_t)nb * (ad.Ha + 1));
    if (!*ga) return -12;
    *gb = *ga + nb * ad.Ha; *nblk = (int)nb;
    RC(fill_zero(*ga, nb * (ad.Ha + 1), st));          // workgroups behind an event's end return early: their rows stay zero
    float* dps = nullptr;
    if (!rows_disjoint) { dps = det_scratch(DET_DPALL, (size_t)ad.N * ad.A * ad.Ha); if (!dps) return -12; }
    RC(launch_att_post(ad, PALL, QS, alpha, DSC, ev_start, ev_len, dps ? dps : DPALL, *ga, *gb, S, dps ? 2 : 1, st, 1));
    if (dps) {
        hipLaunchKernelGGL(dpall_fold_kernel, dim3(Tv), dim3(256), 0, st, dps, ev_start, ev_len, DPALL, ad.N, ad.A, ad.Ha);
        RC(check_launch("dpall_fold"));
    }
    return 0;
}
int att_post_launch(const AttShape& s, int Tv, int S, int rows_disjoint, const float* PALL, const float* QS, const float* alpha, const float* DSC,
                    const int* ev_start, const int* ev_len, float* DPALL, float* GAREP, float* GBREP, float* g_alpha, float* g_balpha, hipStream_t st) {
    const AttDims ad{s.N, s.A, s.Ha, s.D};
    const int Ha = s.Ha;
    if (det_mode()) {
        float *ga, *gb; int nblk;
        RC(att_post_fixed_order(ad, Tv, S, rows_disjoint, PALL, QS, alpha, DSC, ev_start, ev_len, DPALL, &ga, &gb, &nblk, st));
        RC(colsum(ga, Ha, nblk, Ha, g_alpha, true, st));
        return colsum(gb, 1, nblk, 1, g_balpha, true, st);
    }
    RC(launch_att_post(ad, PALL, QS, alpha, DSC, ev_start, ev_len, DPALL, GAREP, GBREP, S, rows_disjoint ? 1 : 0, st));
    RC(colsum(GAREP, Ha, ALPHA_REP, Ha, g_alpha, true, st));
    return colsum(GBREP, 1, ALPHA_REP, 1, g_balpha, true, st);
}
int att_check_dims(const AttShape& s, const char* who) {
    ECHR_REQUIRE(s.D % 4 == 0 && s.Ha % 4 == 0 && s.Ha <= 256 * MAXR && s.D <= 256 * MAXR && s.D >= 4 && s.Ha >= 4,
                 "%s: need D%%4==0, Ha%%4==0, 4 <= D,Ha <= %d (D=%d Ha=%d)", who, 256 * MAXR, s.D, s.Ha);
    return 0;
}

}  // namespace echr

using namespace echr;

extern "C" int64_t echr_batch_ws_floats(int32_t N, int32_t n_videos, int32_t H) {
    return (N > 0 && n_videos > 0 && n_videos <= N && H > 0) ? carve_batch(N, n_videos, H, nullptr).total : -1;
}
extern "C" int64_t echr_decoder_ws_floats(const echr_dec_args* a) { return a ? carve_ws(a, nullptr).total : -1; }
extern "C" int64_t echr_decoder_ws_bwd_floats(const echr_dec_args* a) { return a ? carve_ws_bwd(a, nullptr).total : -1; }

extern "C" int echr_stream_join(void* stream) { return join_tail((hipStream_t)stream); }


// ---- event-independent part of the decoder forward, ahead of (and concurrent with) the event encoder ----
struct Prep { hipStream_t s = nullptr; hipEvent_t fork = nullptr, done = nullptr, fill_done = nullptr, fill0 = nullptr; bool ok = false, init = false, pending = false, fill_pending = false; const void* ws = nullptr; };
static Prep& prep() {
    static Prep t;
    if (!t.init) {
        t.init = true;
        bool good = hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.fork, echr::sync_event_flags()) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.done, echr::sync_event_flags()) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.fill_done, echr::sync_event_flags()) == hipSuccess;
        good = good && hipEventCreateWithFlags(&t.fill0, echr::sync_event_flags()) == hipSuccess;
        t.ok = good;
    }
    return t;
}
// the prepare stream outside a forward pass (idle during the backward pass): a second helper stream for work that is independent of what the
// caller's stream and the tail stream carry (the decoder backward's LSTM-layer stage).  fork: it continues after everything
// queued on `from`; join: `to` waits for what was queued on it since.  nullptr / no-op when unavailable or when a prepare is pending.
namespace echr {
hipStream_t aux2_fork(hipStream_t from) {
    Prep& pr = prep();
    if (!pr.ok || pr.pending) return nullptr;
    if (hipEventRecord(pr.fork, from) != hipSuccess || hipStreamWaitEvent(pr.s, pr.fork, 0) != hipSuccess) return nullptr;
    return pr.s;
}
int aux2_join(hipStream_t to) {
    Prep& pr = prep();
    if (hipEventRecord(pr.done, pr.s) != hipSuccess || hipStreamWaitEvent(to, pr.done, 0) != hipSuccess) { set_error("stream join failed"); return -5; }
    return 0;
}
// echr_train_step's joint mode (step.hip): the helper streams keep working after the call returns
bool helpers_available() { return tail().ok && prep().ok && !prep().pending; }
}  // namespace echr
// see include/echr_hip.h: the helper streams are created in a fixed order and each submits a marker, so that their hardware queues are
// assigned before any other component (RCCL) creates streams of its own
extern "C" int echr_streams_init(void) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); set_error("streams_init: no device"); return -19; }
    // (the two helper streams: with the caller's stream and the collective library's they fill this runtime's four hardware queues)
    Tail& t = tail();
    Prep& p = prep();
    bool ok = true;
    if (t.ok) ok = ok && hipEventRecord(t.fork, t.s) == hipSuccess && hipStreamSynchronize(t.s) == hipSuccess;
    if (p.ok) ok = ok && hipEventRecord(p.fork, p.s) == hipSuccess && hipStreamSynchronize(p.s) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); set_error("streams_init: marker submission failed"); return -5; }
    return 0;
}
namespace echr {
hipStream_t aux2_stream() { return prep().ok ? prep().s : nullptr; }
hipStream_t tail_stream_raw() { return tail().ok ? tail().s : nullptr; }
int prep_stream_wait(hipEvent_t ev) {
    Prep& pr = prep();
    if (!pr.ok || hipStreamWaitEvent(pr.s, ev, 0) != hipSuccess) { set_error("prepare stream wait failed"); return -5; }
    return 0;
}
hipStream_t helpers_merge_to_tail() {          // the tail stream continues behind everything queued on the prepare stream; returns the tail stream
    Tail& t = tail();
    Prep& pr = prep();
    if (hipEventRecord(pr.done, pr.s) != hipSuccess || hipStreamWaitEvent(t.s, pr.done, 0) != hipSuccess) { set_error("stream join failed"); return nullptr; }
    return t.s;
}
int tail_publish() {                           // what the tail stream carries now is what echr_stream_join / the next library call waits for
    Tail& t = tail();
    if (hipEventRecord(t.done, t.s) != hipSuccess) { set_error("event record failed"); return -5; }
    t.pending = true;
    t.pending3 = false;
    return 0;
}
}  // namespace echr
// will echr_decoder_fwd run the persistent forward launch on these arguments (same test as there)?
static bool fwd_uses_persist(const echr_dec_args* a) { return persist_fwd_eligible(a); }
static int decoder_fill(const echr_dec_args* a, const DecWs& w, hipStream_t st, bool with_extra = true) {
    const int N = a->N, S = a->S, H = a->H;
    // h(-1) = c(-1) = 0 (init_hidden, :75-78), the atomic q accumulators and the split-K target EVB0 -- and the zeroed part of the persistent
    // launch's exchange workspace (counters, accumulated buffers): one launch
    float* zp[8] = {w.HS, w.CS[0], w.CS[1], w.CS[2], w.QACC, w.EVB0, nullptr, nullptr};
    long zn[8] = {(long)N * 3 * H, (long)N * H, (long)N * H, (long)N * H, (long)S * N * a->Ha, (long)N * 4 * H, 0, 0};
    int n = 6;
    if (fwd_uses_persist(a)) { persist_fwd_zero_range(a, w.XWS, &zp[n], &zn[n]); ++n; }
    if (with_extra && a->zero_extra && a->zero_extra_count > 0) { zp[n] = a->zero_extra; zn[n] = (long)a->zero_extra_count; ++n; }      // the caller's gradient arena
    return fill_zero_multi(zp, zn, n, st);
}

// the backward pass's zero-initialised scratch: DC | DGCOL | DHACC | DQ | DASL | DPALL, the split-K / accumulated outputs DXT, g_event and DOUT,
// the zeroed part of the persistent reverse launch's exchange workspace and, when the caller asks for it (zero_extra), its gradient arena span
static int bwd_scratch_ranges(const echr_dec_args* a, const echr_dec_grads* g, const DecWsBwd& b, bool bwd_persist, float** zp, long* zn) {
    const long SN = (long)a->S * a->N;
    zp[0] = b.DC; zn[0] = b.zero_floats;
    zp[1] = b.DXT; zn[1] = SN * a->E;
    zp[2] = g->g_event; zn[2] = (long)a->N * a->De;
    zp[3] = b.DOUT; zn[3] = SN * 3 * a->H;
    int nz = 4;
    if (bwd_persist) { persist_bwd_zero_range(a, b.XWSB, &zp[nz], &zn[nz]); ++nz; }
    if (g->zero_extra && g->zero_extra_count > 0) { zp[nz] = g->zero_extra; zn[nz] = (long)g->zero_extra_count; ++nz; }
    return nz;
}
// the backward workspace whose scratch fill echr_train_step has already queued behind the decoder's prepare (nullptr: none)
static const void*& scratch_ahead() { static const void* p = nullptr; return p; }
namespace echr {
// echr_train_step, right after echr_decoder_fwd_prepare: the backward pass's scratch fill (32 MB) joins the gradient-arena fill at the end of
// the prepare stream -- long before the backward pass, beside the forward recurrence -- instead of being a launch of its own between the two
// recurrences; echr_decoder_bwd then skips its fill (it waits for the prepare stream's fill event on entry anyway)
int decoder_bwd_scratch_ahead(const echr_dec_args* a, const echr_dec_grads* g) {
    Prep& pr = prep();
    if (!pr.ok || !pr.pending || !pr.fill_pending || pr.ws != a->ws || !g->ws_bwd || !g->g_event) return 0;
    const DecWsBwd b = carve_ws_bwd(a, g->ws_bwd);
    const bool bwd_persist = persist_bwd_eligible(a);
    float* zp[FILL_MAX_JOBS];
    long zn[FILL_MAX_JOBS];
    echr_dec_grads gz = *g;
    gz.zero_extra = nullptr; gz.zero_extra_count = 0;
    const int nz = bwd_scratch_ranges(a, &gz, b, bwd_persist, zp, zn);
    RC(fill_zero_multi(zp, zn, nz, pr.s));
    if (hipEventRecord(pr.fill_done, pr.s) != hipSuccess) { set_error("event record failed"); return -5; }
    scratch_ahead() = g->ws_bwd;
    return 0;
}
}  // namespace echr
extern "C" int echr_decoder_fwd_prepare(const echr_dec_args* a, void* stream) { return decoder_fwd_prepare(a, DecCall{}, stream); }
int echr::decoder_fwd_prepare(const echr_dec_args* a, const DecCall& c, void* stream) {
    RC(persist_check_async());
    RC(check_dims(a, "decoder_fwd_prepare"));
    ECHR_REQUIRE(a->S > 0 && a->ws && a->tokens, "decoder_fwd_prepare: missing buffers");
    Prep& pr = prep();
    ECHR_REQUIRE(pr.ok, "decoder_fwd_prepare: stream state unavailable");
    hipStream_t sm = (hipStream_t)stream, st = pr.s;
    scratch_ahead() = nullptr;          // (a train step whose backward never ran)
    RC(echr_decoder_fwd_prepare_cancel(stream));          // an earlier prepare nobody consumed: order its workspace before anything new
    RC(join_tail(sm));
    if (hipEvent_t fe = fork_event_slot()) {
        if (hipStreamWaitEvent(st, fe, 0) != hipSuccess) { set_error("decoder_fwd_prepare: stream fork failed"); return -5; }
    } else RC(hop(sm, pr.fork, st));
    DecWs w = carve_ws(a, a->ws, c.bx, c.scene_rows);
    // the persistent forward chain's weight images (parameters only) are built now, on the CALLER's stream -- it idles ~20 us waiting for the
    // position branch's gates -- so that the launch copies them instead of converting them in front of its first step (set-up 24.7 -> ~14 us)
    if (fwd_uses_persist(a)) RC(persist_fwd_prebuild(a, w.XWS, sm));
    // the caller's gradient arena (echr_train_step: 87 MB) is zero-filled LAST on this stream, behind the event this call publishes: nothing of
    // the forward pass waits for it -- a fill has no LDS and a handful of registers, so it also fits beside the recurrence's workgroups -- and
    // echr_decoder_bwd waits for it on entry.  -10 us per iteration against the fill in front (A/B: 1.540 vs 1.550 ms)
    const bool late = a->zero_extra && a->zero_extra_count > 0;
    RC(decoder_fill(a, w, st, !late));
    // (the event-context gate product of echr_decoder_fwd accumulates into EVB0, zeroed by this fill: it waits for THIS event, not for the
    // whole chain below -- the product then runs beside the chain's last GEMM instead of behind it)
    if (hipEventRecord(pr.fill0, st) != hipSuccess) { set_error("decoder_fwd_prepare: event record failed"); return -5; }
    // the two W_logit images are packed on the caller's stream, not at the head of the prepare chain: it has slack in front of the recurrence
    // since the position branch starts beside the previous update (stage-ahead): 1.450-1.454 vs 1.445-1.465 ms and 1.414-1.422 vs 1.418-1.431
    // on two boxes (-5 us in the mean)
    RC(precompute_static(a, w, st, true, true, 1, sm));
    RC(embed_gather(a->embed, a->tokens, w.XT, a->S * a->N, a->E, a->V1, st));
    RC(input_gates(a, w, w.XT, 0, a->S, st, true));
    if (hipEventRecord(pr.done, st) != hipSuccess) { set_error("decoder_fwd_prepare: event record failed"); return -5; }
    pr.pending = true; pr.ws = a->ws;
    if (late) {          // the caller's gradient arena: behind everything the forward recurrence waits for
        RC(fill_zero(a->zero_extra, (long)a->zero_extra_count, st));
        if (hipEventRecord(pr.fill_done, st) != hipSuccess) { set_error("decoder_fwd_prepare: event record failed"); return -5; }
        pr.fill_pending = true;
    }
    return 0;
}

extern "C" int echr_decoder_fwd_prepare_cancel(void* stream) {
    Prep& pr = prep();
    if (!pr.ok || !pr.pending) return 0;
    pr.pending = false; pr.ws = nullptr;
    if (hipStreamWaitEvent((hipStream_t)stream, pr.done, 0) != hipSuccess) { set_error("decoder_fwd_prepare_cancel: join failed"); return -5; }
    return 0;
}

static int decoder_fwd_impl(const echr_dec_args* a, const echr_dropout* drop, void* stream, const echr_dec_grads* fz, bool* fused_out, bool* compact_out,
                            const DecCall& c);
extern "C" int echr_decoder_fwd(const echr_dec_args* a, const echr_dropout* drop, void* stream) { return decoder_fwd_impl(a, drop, stream, nullptr, nullptr, nullptr, DecCall{}); }
namespace echr {
int decoder_fwd_fused(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream, bool* fused, bool* compact, const DecCall& c) {
    return decoder_fwd_impl(a, drop, stream, g, fused, compact, c);
}
int decoder_fused_loss(const echr_dec_args* a, const echr_dec_grads* g, float* loss, hipStream_t st, bool rw, bool unit_den) {
    const DecWsBwd b = carve_ws_bwd(a, g->ws_bwd);
    return nll_rows_sum(b.ROWL, (g->active_rows && g->n_active > 0) ? g->n_active : a->S * a->N, b.MSUM, loss, st, rw, unit_den);
}
}  // namespace echr
// fz != nullptr: the criterion is fused behind the logits product (echr_train_step) -- the logits are turned into d logits in ws_bwd and
// per-row loss terms by ONE pass instead of log-softmax, NLL and log-softmax backward passes; the log-probs are never materialised
// c.rw (with fz): RewardCriterion's signed weight [N,S] (echr_train_step_rw) in place of the NLL's mask in the fused criterion pass, over the
// denominator 1 when the call is a batch (c.bx)
static int decoder_fwd_impl(const echr_dec_args* a, const echr_dropout* drop, void* stream, const echr_dec_grads* fz, bool* fused_out, bool* compact_out,
                            const DecCall& c) {
    if (fused_out) *fused_out = false;
    if (compact_out) *compact_out = false;
    RC(persist_check_async());
    RC(join_tail((hipStream_t)stream));
    RC(check_dims(a, "decoder_fwd"));
    ECHR_REQUIRE(a->S > 0 && a->ws && a->logp && a->tokens, "decoder_fwd: missing buffers");
    hipStream_t st = (hipStream_t)stream;
    const int N = a->N, S = a->S, H = a->H, E = a->E;
    DecWs w = carve_ws(a, a->ws, c.bx, c.scene_rows);
    const DropCfg dh = make_drop(drop, drop ? drop->p_h : 0.f), dout = make_drop(drop, drop ? drop->p_out : 0.f);
    bool evb0_pending = false;
    if (a->prepared) {
        // echr_decoder_fwd_prepare already ran everything that does not need the event context on the library's second stream
        Prep& pr = prep();
        ECHR_REQUIRE(pr.ok && pr.pending && pr.ws == a->ws, "decoder_fwd: prepared = 1 without a matching echr_decoder_fwd_prepare on this workspace");
        pr.pending = false;
        if (hipStreamWaitEvent(st, pr.fill0, 0) != hipSuccess) { set_error("decoder_fwd: join failed"); return -5; }
        RC(precompute_static(a, w, st, true, true, 2));
        if (hipStreamWaitEvent(st, pr.done, 0) != hipSuccess) { set_error("decoder_fwd: join failed"); return -5; }
        evb0_pending = fwd_uses_persist(a) && persist_fwd_adds_evb0();      // the persistent launch's LSTM role adds the event part itself
        if (!evb0_pending) {
            const long n4 = (long)S * N * H;            // 4H / 4 float4 per row
            hipLaunchKernelGGL(add_bcast_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, w.GATES[0], w.EVB0, (long)S * N, (long)N, H);
            RC(check_launch("add_bcast_rows"));
        }
    } else {
        RC(decoder_fill(a, w, st));
        RC(precompute_static(a, w, st, true, true));
        RC(embed_gather(a->embed, a->tokens, w.XT, S * N, E, a->V1, st));
        RC(input_gates(a, w, w.XT, 0, S, st));
    }
    if (a->h0) RC(init_state_copy(a, w, st));          // OldModel.init_hidden with CG_init_feats_type (:79-96): behind the zero fill of HS[0] / CS[k][0]
    // late fusion: logits = OUTD . W_logit^T + b, written [N,S,V1], then row log-softmax in place, behind the recurrence
    auto logits = [&](hipStream_t q) -> int {
        // echr_train_step with the criterion's active rows: logits only for the rows that can reach the loss (compact [n_active, V1] in the
        // log-prob buffer, which nothing else reads on that path), then log-softmax + criterion + d logits in one pass over them
        if (fz && fz->active_rows && fz->n_active > 0 && fz->nll_target && fz->nll_mask && fz->g_loss && fz->ws_bwd) {
            const DecWsBwd b = carve_ws_bwd(a, fz->ws_bwd);
            if (logsoftmax_nll_dlg_ok(a->V1, b.ldg)) {
                echr_gemm_desc dc;
                if (config().gemm_h2) {
                H2PackJob pj = pack_rows(w.OUTD, 3 * H, fz->n_active, 3 * H, w.PK_OUTD);
                pj.gather = fz->active_rows;
                RC(h2_pack_multi(&pj, 1, q));
                dc = desc_h2(w.PK_OUTD, w.PK_WL, a->logp, a->V1, fz->n_active, a->V1, 3 * H);
                dc.split_k = 1;
                } else {
                // native fp32 / bf16x3 products: the active rows are gathered into a dense [n_active, 3H] operand (in the region the h2
                // path packs into; the backward pass reads it again for d W_logit) and the products run on n_active rows
                RC(embed_gather(w.OUTD, fz->active_rows, w.PK_OUTD, fz->n_active, 3 * H, S * N, q));
                dc = desc_nt(w.PK_OUTD, 3 * H, a->w_logit, 3 * H, a->logp, a->V1, fz->n_active, a->V1, 3 * H);
                dc.algo = ECHR_GEMM_BF16X3;
                }
                dc.bias = a->b_logit;
                RC(gemm(dc, q));
                if (fused_out) *fused_out = true;
                if (compact_out) *compact_out = true;
                return logsoftmax_nll_dlg(a->logp, a->V1, fz->nll_target, fz->nll_target_i64, fz->nll_mask, fz->g_loss, b.DLG, b.ldg, b.ROWL, b.MSUM, N, S, a->V1, q,
                                          fz->active_rows, fz->n_active, c.rw, c.bx != nullptr);
            }
        }
        echr_gemm_desc d = desc_nt(w.OUTD, 3 * H, a->w_logit, 3 * H, a->logp, a->V1, S * N, a->V1, 3 * H);
        d.algo = ECHR_GEMM_BF16X3;
        if (config().gemm_h2) {
            H2PackJob pj = pack_rows(w.OUTD, 3 * H, S * N, 3 * H, w.PK_OUTD);
            RC(h2_pack_multi(&pj, 1, q));
            d = desc_h2(w.PK_OUTD, w.PK_WL, a->logp, a->V1, S * N, a->V1, 3 * H);
            d.split_k = 1;
        }
        d.bias = a->b_logit; d.rowmap_mod = N; d.rowmap_mul = S;
        RC(gemm(d, q));
        if (fz && fz->nll_target && fz->nll_mask && fz->g_loss && fz->ws_bwd) {
            const DecWsBwd b = carve_ws_bwd(a, fz->ws_bwd);
            if (logsoftmax_nll_dlg_ok(a->V1, b.ldg)) {
                if (fused_out) *fused_out = true;
                return logsoftmax_nll_dlg(a->logp, a->V1, fz->nll_target, fz->nll_target_i64, fz->nll_mask, fz->g_loss, b.DLG, b.ldg, b.ROWL, b.MSUM, N, S, a->V1, q,
                                          nullptr, 0, c.rw, c.bx != nullptr);
            }
        }
        return logsoftmax_rows(a->logp, a->V1, N, S, 0, S, a->V1, q);
    };
    if (persist_fwd_eligible(a)) {
        // all S timesteps in ONE persistent launch: recurrent weights stay in LDS, attention operands in registers (csrc/persist.hip)
        PersistFwdBufs pb;
        for (int k = 0; k < 3; ++k) { pb.GATES[k] = w.GATES[k]; pb.CS[k] = w.CS[k]; }
        pb.HS = w.HS; pb.OUTD = w.OUTD; pb.QS = w.QS; pb.WT = w.WT; pb.ATT = w.ATT; pb.PALL = w.PALL; pb.xws = w.XWS;
        pb.prezeroed = true;                    // decoder_fill covered the exchange workspace's zeroed part
        if (evb0_pending) pb.EVB0 = w.EVB0;
        RC(persist_fwd(a, pb, dh, dout, st));
    } else {
        for (int t = 0; t < S; ++t) RC(step_fwd(a, w, t, dh, dout, st, true));
    }
    return logits(st);
}

extern "C" int echr_decoder_bwd(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream) {
    return echr::decoder_bwd_checked(a, g, drop, stream, DecCall{});
}
// ---- multi-video batches: the single-video code, called with the extension (DecCall.bx) ----
static DecCall dec_batch_call(const echr_batch_ext* x, bool scene_rows = false) { DecCall c; c.bx = x; c.scene_rows = scene_rows; return c; }
static int check_batch(const echr_dec_args* a, const echr_batch_ext* x, const char* who) {
    ECHR_REQUIRE(a && x && x->n_videos > 0 && x->n_videos <= a->N && x->vid && x->video && x->ws, "%s: the batch extension needs 0 < n_videos <= N, vid, video and ws", who);
    return 0;
}
extern "C" int echr_decoder_fwd_batch(const echr_dec_args* a, const echr_dropout* drop, const echr_batch_ext* x, void* stream) {
    RC(check_batch(a, x, "decoder_fwd_batch"));
    ECHR_REQUIRE(!a->prepared, "decoder_fwd_batch: prepared must be 0");
    return decoder_fwd_impl(a, drop, stream, nullptr, nullptr, nullptr, dec_batch_call(x));
}
extern "C" int echr_decoder_bwd_batch(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, const echr_batch_ext* x, void* stream) {
    RC(check_batch(a, x, "decoder_bwd_batch"));
    return echr::decoder_bwd_checked(a, g, drop, stream, dec_batch_call(x));
}
namespace echr {
int decoder_fused_video_loss(const echr_dec_args* a, const echr_dec_grads* g, const int* vid, int V, float* vloss, hipStream_t st) {
    const DecWsBwd b = carve_ws_bwd(a, g->ws_bwd);
    const bool compact = g->active_rows && g->n_active > 0;
    return video_loss_rows(b.ROWL, compact ? g->active_rows : nullptr, compact ? g->n_active : a->S * a->N, a->N, vid, V, vloss, st);
}
}  // namespace echr
int echr::decoder_bwd_checked(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream, const DecCall& c) {
    RC(persist_check_async());
    RC(join_tail((hipStream_t)stream));
    RC(check_dims(a, "decoder_bwd"));
    ECHR_REQUIRE(g && a->ws && g->ws_bwd && a->logp, "decoder_bwd: missing buffers");
    ECHR_REQUIRE(g->dlg_ready || g->g_logp || (g->nll_target && g->nll_mask && g->g_loss), "decoder_bwd: need g_logp or the fused NLL inputs");
    return decoder_bwd_parts(a, g, drop, stream, 0, c);
}

// ---- decoder backward: one plan (BwdPlan, made at entry, before the first launch), stages as functions of (plan, stream), two schedulers
// (bwd_lstm_stage, bwd_tail_stage).  No stage reassigns its stream; what one scheduler leaves for the other travels in BwdSched.
// Which stage runs on which stream.  C = the caller's stream, T = the tail stream, P = the prepare stream (idle during a backward pass); head =
// d logits + scratch + late fusion, rec = reverse recurrence (+ d h0), lstm = weight gradients, bias sums, d W_ih0[:, E:], scene gradients, wl =
// logit-layer gradients, att = attention parameters, emb = embedding chain:
//   schedule                     head          rec    d event  lstm   wl               att    emb    forks / joins
//   synchronous (also phase 2)   C (with wl)   C      C        C      C, inside head   C      C      none
//   async_tail 1                 C             C      C        C      T                T      T      T forks behind lstm (tail().fork); tail().done
//   async_tail 2 (zeroed)        C             C      C        P      T                T      P      P and T fork behind rec off ONE event (prep().fork), P sums
//                                                                                                   d gates0 per event itself; tail().done3 / tail().done
//   staged phases 1 / 3 / 4      C, phase 1    C, 3   C, 3     C, 3   C, inside head   C, 4   C, 4   none
//   two-piece parts 1 / 2        C, part 1     C, 1   C, 1     P, 2   T, 2             T, 2   P, 2   part 2 forks P and T where it is called; done3 / done
// async_tail needs phase 0 and the tail stream, else the call is synchronous; async_tail 2 without zeroed gradients runs as async_tail 1; without the
// prepare stream (a prepare is pending) lstm follows d event on C and emb moves to T.  Deferred wl on the native product path needs part 0.  A
// data-parallel hand-over point is marked behind wl (on T) and behind lstm (on P).  part 0 is the whole call; the two pieces are echr_train_step's
// joint mode (d tap_feats wanted early, step.hip): part 2 is called, and forks, behind the event encoder's backward.  Pieces need async_tail = 2.
enum { BWD_HEAD = 1, BWD_REC = 2, BWD_LSTM = 4, BWD_TAIL = 8 };          // the stage mask of a call
enum { EV_SUMS = 1, EV_D_WEIGHT = 2, EV_D_EVENT = 4 };                      // what bwd_event_grads forms, in this order
struct BwdPlan {
    const echr_dec_args* a; const echr_dec_grads* g;
    DecCall c;          // the call: criterion weight, batch extension (also in w), hand-over request (in force only when the events exist)
    int part, N, S, H, E, Ha, A, D, V1, SN, cin[3];
    DecWs w; DecWsBwd b; DropCfg dh, dout;
    bool z, h2; float zb;          // z: gradient buffers pre-zeroed by the caller: accumulate (beta zb = 1), no fills; h2: products on h2-packed operands
    // echr_train_step's compacted late-fusion stage: d logits exist for the SNc rows with a non-zero criterion mask only (rows act[i]);
    // crec: the recurrent weight gradients / d XT on the active rows too (the k gather rides in the h2 packs: the native products keep all rows)
    bool compact, crec; int SNc, SNr; const int *act, *actr;
    bool bwd_persist;              // the reverse recurrence runs as the persistent launch (same test as the recurrence stage applies)
    int stages;                    // BWD_*: late fusion | reverse recurrence | its batched parameter gradients | attention + embedding gradients
    bool defer_wl;                 // the logit-layer gradients, which nothing in the backward pass reads, are formed on the tail stream
    bool lstm_on_helper;           // async_tail = 2: only d event on the caller's stream, the rest of the LSTM-layer stage on the prepare stream
    bool async_tail;               // the tail stage runs on the tail stream, joined by the caller
    const float* outd_rows;        // native + compact: the forward's gathered [n_active, 3H] operand
};
struct BwdSched { bool embed_queued = false, bias_owed = false; };          // embedding chain already queued (prepare stream) | d b_logit still owed (tail)
// Every check that needs no launch result, before the first launch: a refused call queues nothing.
static int bwd_plan(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, int part, const DecCall& c, BwdPlan& p) {
    ECHR_REQUIRE(part == 0 || (g->phase == 0 && g->async_tail == 2 && g->zeroed && config().gemm_h2 && tail().ok),
                 "decoder_bwd: the two-piece form needs phase 0, async_tail 2, zeroed gradients, the h2 path and the helper streams");
    p.a = a; p.g = g; p.part = part;
    p.c = c; p.c.handover = c.handover && handover().ok;
    p.N = a->N; p.S = a->S; p.H = a->H; p.E = a->E; p.Ha = a->Ha; p.A = a->A; p.D = a->D; p.V1 = a->V1; p.SN = a->S * a->N;
    p.cin[0] = a->E + a->De; p.cin[1] = a->E + a->D; p.cin[2] = a->E + a->Dv;
    p.w = carve_ws(a, a->ws, c.bx, c.scene_rows); p.b = carve_ws_bwd(a, g->ws_bwd);
    p.dh = make_drop(drop, drop ? drop->p_h : 0.f); p.dout = make_drop(drop, drop ? drop->p_out : 0.f);
    p.z = g->zeroed != 0; p.zb = p.z ? 1.f : 0.f; p.h2 = config().gemm_h2 != 0;
    p.compact = g->dlg_ready && g->active_rows && g->n_active > 0; p.crec = p.compact && p.h2;
    p.SNc = p.compact ? g->n_active : p.SN; p.act = p.compact ? g->active_rows : nullptr;
    p.SNr = p.crec ? p.SNc : p.SN; p.actr = p.crec ? p.act : nullptr;
    ECHR_REQUIRE(!p.compact || (g->phase == 0 && g->async_tail != 0), "decoder_bwd: active_rows needs the asynchronous tail");
    ECHR_REQUIRE(g->phase >= 0 && g->phase <= 4, "decoder_bwd: phase must be 0..4");
    const int all = BWD_HEAD | BWD_REC | BWD_LSTM | BWD_TAIL;
    const int by_phase[5] = {all, BWD_HEAD, BWD_REC | BWD_LSTM | BWD_TAIL, BWD_REC | BWD_LSTM, BWD_TAIL};
    p.stages = by_phase[g->phase] & (part == 1 ? BWD_HEAD | BWD_REC | BWD_LSTM : part == 2 ? BWD_LSTM | BWD_TAIL : all);
    const bool tail_ok = g->phase == 0 && g->async_tail != 0 && tail().ok;
    p.defer_wl = tail_ok && (p.h2 || part == 0);
    p.lstm_on_helper = p.defer_wl && g->async_tail == 2 && p.z;
    p.async_tail = tail_ok && (p.stages & BWD_TAIL);
    ECHR_REQUIRE(p.h2 || !p.compact || p.defer_wl, "decoder_bwd: active_rows on the native product path needs the deferred logit-layer gradients");
    ECHR_REQUIRE(!(p.stages & BWD_HEAD) || !p.h2 || !p.compact || p.defer_wl, "decoder_bwd: active_rows needs the deferred logit-layer gradients");
    p.bwd_persist = persist_bwd_eligible(a); p.outd_rows = (p.compact && !p.h2) ? p.w.PK_OUTD : p.w.OUTD;
    return 0;
}
// 1. d logits (time-major, padded leading dimension), the transposed recurrent weights and the zero-filled scratch
static int bwd_dlogits_and_scratch(const BwdPlan& p, hipStream_t st) {
    const echr_dec_args* a = p.a; const echr_dec_grads* g = p.g; const DecWsBwd& b = p.b; const int N = p.N, S = p.S, H = p.H, E = p.E, V1 = p.V1;
    if (!g->dlg_ready) {          // (echr_train_step formed d logits in the pass that read the logits)
        if (!g->g_logp && !g->nll_msum) RC(colsum(g->nll_mask, 1, N * S, 1, b.MSUM, false, st));
        RC(logsoftmax_bwd(a->logp, g->g_logp, g->nll_target, g->nll_target_i64, g->nll_mask, g->g_loss, g->nll_msum ? g->nll_msum : b.MSUM, b.DLG, b.ldg, N, S, V1, st,
                           p.c.rw, p.c.bx != nullptr));
    }
    // scratch that is accumulated into, and the transposed recurrent weights (every d h / d ATT product of the reverse recurrence
    // then has the same NT form as forward): two launches, independent of everything above
    // (the persistent reverse launch builds its weight images from the untransposed matrices: nothing to transpose then)
    if (!p.bwd_persist) {
        const TransposeJob tj[5] = {{a->w_hh[0], H, b.WT_HH[0], 4 * H, 4 * H, H}, {a->w_hh[1], H, b.WT_HH[1], 4 * H, 4 * H, H},
                                    {a->w_hh[2], H, b.WT_HH[2], 4 * H, 4 * H, H}, {a->w_ih[1] + E, p.cin[1], b.WT_ATT, 4 * H, 4 * H, p.D},
                                    {a->w_h2a, H, b.WT_H2A, p.Ha, p.Ha, H}};
        RC(transpose_multi(tj, 5, st));
    }
    if (scratch_ahead() == g->ws_bwd && g->dlg_ready) {
        // echr_train_step queued this fill behind the decoder's prepare (decoder_bwd_scratch_ahead); this stream waited for it on entry
        if (g->zero_extra && g->zero_extra_count > 0) RC(fill_zero(g->zero_extra, (long)g->zero_extra_count, st));
    } else {
        float* zp[FILL_MAX_JOBS]; long zn[FILL_MAX_JOBS];
        RC(fill_zero_multi(zp, zn, bwd_scratch_ranges(a, g, b, p.bwd_persist, zp, zn), st));
    }
    scratch_ahead() = nullptr;
    return 0;
}
// d W_logit = DLG^T . OUTD and d b_logit over the SNc rows of d logits: on h2-packed operands that the caller has prepared (a plain overwrite), or
// on the native path through transposes.  bias_too = false: the caller folds the column sum of DLG into a later multi-problem column-sum launch
static int bwd_logit_grads(const BwdPlan& p, hipStream_t st, bool bias_too = true) {
    const echr_dec_grads* g = p.g; const DecWsBwd& b = p.b; const int H = p.H, V1 = p.V1, SNc = p.SNc;
    echr_gemm_desc d;
    if (p.h2) {
        d = desc_h2(b.PK_DLGT, b.PK_OUTDT, g->g_w_logit, 3 * H, V1, 3 * H, SNc);
        d.split_k = 1;                         // one k slice per tile: a plain overwrite, no read of the (zeroed or stale) 30 MB buffer
    } else {
        // (compact: SNc rows of d logits against the gathered OUTD rows; the transposes zero-pad the contraction to its padded length)
        const int kp = (SNc + 3) / 4 * 4;
        RC(transpose(b.DLG, b.ldg, b.DLGT, b.snp, SNc, V1, kp, st));
        RC(transpose(p.outd_rows, 3 * H, b.OUTDT, b.snp, SNc, 3 * H, kp, st));
        d = desc_nt(b.DLGT, b.snp, b.OUTDT, b.snp, g->g_w_logit, 3 * H, V1, 3 * H, kp);
        d.beta = p.zb; d.split_k = -1; d.algo = ECHR_GEMM_BF16X3;
    }
    RC(gemm(d, st));
    return bias_too ? colsum(b.DLG, b.ldg, SNc, V1, g->g_b_logit, p.z, st) : 0;
}
// 2. late fusion gradients.  Both late-fusion products run as NT problems on k-contiguous (transposed) operands so that they qualify for the
// bf16-split matrix-core path: d W_logit = DLG^T . OUTD  and  d OUTD = DLG . W_logit.
static int bwd_late_fusion(const BwdPlan& p, hipStream_t st) {
    const echr_dec_args* a = p.a; const DecWs& w = p.w; const DecWsBwd& b = p.b; const int H = p.H, V1 = p.V1, SN = p.SN, SNc = p.SNc;
    echr_gemm_desc d;
    if (p.h2) {
        // d W_logit = DLG^T . OUTD and d OUTD = DLG . W_logit on h2-packed operands; the four packs (two of them transposing) are one launch
        // with an asynchronous tail (phase 0) the logit-layer gradients, which nothing in the backward pass reads, are formed on the tail
        // stream beside the launch-bound rest of the backward instead of in front of the reverse recurrence
        // (a->train: W_logit^T was packed with the forward operands; otherwise here)
        const float* pk_wlt = a->train ? w.PK_WLT : b.PK_WLT;
        if (p.defer_wl) {
            H2PackJob pj[2] = {pack_rows(b.DLG, b.ldg, SNc, V1, b.PK_DLG), pack_cols(a->w_logit, 3 * H, 3 * H, V1, b.PK_WLT)};
            RC(h2_pack_multi(pj, a->train ? 1 : 2, st));
        } else {
            H2PackJob pj[4] = {pack_cols(b.DLG, b.ldg, V1, SN, b.PK_DLGT), pack_cols(w.OUTD, 3 * H, 3 * H, SN, b.PK_OUTDT),
                               pack_rows(b.DLG, b.ldg, SN, V1, b.PK_DLG), pack_cols(a->w_logit, 3 * H, 3 * H, V1, b.PK_WLT)};
            RC(h2_pack_multi(pj, a->train ? 3 : 4, st));
            RC(bwd_logit_grads(p, st));
        }
        d = desc_h2(b.PK_DLG, pk_wlt, b.DOUT, 3 * H, SNc, 3 * H, V1);
    } else {
        // (native fp32 / bf16x3 products.  With an asynchronous tail the logit-layer gradients -- which nothing in the backward pass reads -- are formed
        // on the tail stream behind the reverse recurrence, as on the h2 path, instead of in front of it: 0.2 ms off the caller's stream)
        if (!p.defer_wl) RC(bwd_logit_grads(p, st));          // (not compact then: all SN rows, the contraction padded to b.snp)
        RC(transpose(a->w_logit, 3 * H, b.WLT, b.ldg, V1, 3 * H, (int)b.ldg, st));
        d = desc_nt(b.DLG, b.ldg, b.WLT, b.ldg, b.DOUT, 3 * H, SNc, 3 * H, (int)b.ldg);
        d.split_k = -1; d.algo = p.compact ? ECHR_GEMM_F32 : ECHR_GEMM_BF16X3;
    }
    d.beta = 1.f;                          // DOUT was zeroed with the scratch: the k slices add atomically, no fill launch
    if (p.compact) { d.row_index = p.act; d.row_index_max = SN - 1; }          // compacted row i adds into row act[i] of d OUTD (the others stay zero)
    return gemm(d, st);
}
// the logit-layer gradients that bwd_late_fusion deferred, on the tail stream `st`
static int bwd_logit_grads_on_tail(const BwdPlan& p, hipStream_t st, BwdSched& s) {
    const DecWsBwd& b = p.b; const int H = p.H, V1 = p.V1, SNc = p.SNc;
    if (p.h2) {
        H2PackJob pj[2] = {pack_cols(b.DLG, b.ldg, V1, SNc, b.PK_DLGT), pack_cols(p.w.OUTD, 3 * H, 3 * H, SNc, b.PK_OUTDT)};
        pj[1].gather = p.act;          // (compact: the contraction runs over the active rows of OUTD)
        RC(h2_pack_multi(pj, 2, st));
    }
    // h2 + z: d b_logit rides in the multi-problem column-sum launch behind att_post -- unless the logit layer's range is handed over to a
    // data-parallel collective right here (then the bias sum is formed with the product, so the whole range is final)
    s.bias_owed = p.h2 && p.z && !p.c.handover;
    RC(bwd_logit_grads(p, st, !s.bias_owed));
    return handover_mark(p.c, ECHR_HANDOVER_LOGIT, st);
}
// one reverse timestep
static int bwd_step(const BwdPlan& p, int t, hipStream_t q) {
    const echr_dec_args* a = p.a; const echr_dec_grads* g = p.g; const DecWs& w = p.w; const DecWsBwd& b = p.b; const int N = p.N, H = p.H, Ha = p.Ha, D = p.D;
    const long hs = (long)N * H, as = (long)N * D;
    LstmBwdPtrs P;
    for (int k = 0; k < 3; ++k) {
        P.gates[k] = w.GATES[k] + (long)t * N * 4 * H;
        P.c_prev[k] = w.CS[k] + (long)t * N * H;
        P.c_new[k] = w.CS[k] + (long)(t + 1) * N * H;
        P.dgates[k] = b.DG[k] + (long)t * N * 4 * H;
        P.dh_acc[k] = b.DHACC[k];                           // d h(t), added atomically while processing step t+1 (zero at t = S-1)
        P.dh_slab[k] = nullptr; P.nslab[k] = 0; P.kmap[k] = k;
    }
    P.slab_stride = hs;
    hipLaunchKernelGGL(lstm_pointwise_bwd_kernel, dim3((N * H + 255) / 256, 3), dim3(256), 0, q, P,
                       b.DOUT + (long)t * N * 3 * H, b.DC, N, H, t, p.dh, p.dout);
    RC(check_launch("lstm_pointwise_bwd"));
    // d h(t-1) = dG_k(t) . W_hh_k  (skipped at t = 0 when h(-1) is the constant zero state; with echr_dec_args.h0 it is d h0);  d ATT = dG_1(t) . W_ih1[:,E:]
    const bool rec0 = t > 0 || (a->h0 && g->g_h0);
    RecArgs ra; ra.M = N; ra.njobs = 0;
    float* datt = b.DASL + (long)t * N * D;     // re-read by every attention workgroup of an event: one atomically summed buffer
    ra.job[ra.njobs++] = mkjob(P.dgates[1], 4 * H, 4 * H, b.WT_ATT, 4 * H, D, datt, as, D, 1);
    if (rec0)
        for (int k = 0; k < 3; ++k) ra.job[ra.njobs++] = mkjob(P.dgates[k], 4 * H, 4 * H, b.WT_HH[k], 4 * H, H, b.DHACC[k], hs, H, 1);
    RC(rec_gemm(ra, q));
    // attention backward (needed at every t: feeds d P_all, d alpha, d W_h)
    float* dq = b.DQ + (long)t * N * Ha;
    {
        ProfScope prof(PROF_ATT_BWD, 4.0 * N * p.A * (Ha + D), 4.0 * ((double)N * p.A * (Ha + D + 2) + (double)N * (2 * Ha + 2 * D)), q);
        const AttDims ad{N, p.A, Ha, D};
        RC(launch_att_bwd(ad, w.PALL, a->c3d, w.QS + (long)t * N * Ha, a->w_alpha, w.WT + (long)t * N * p.A, w.ATT + (long)t * N * D,
                          datt, 1, as, a->ev_start, a->ev_len, b.DSC + (long)t * N * p.A, dq, q));
    }
    if (rec0) {   // d h1(t-1) += dq . W_h : extra slabs behind stream 1's W_hh slabs
        ra.njobs = 1;
        ra.job[0] = mkjob(dq, Ha, Ha, b.WT_H2A, Ha, H, b.DHACC[1], hs, H, 1);
        RC(rec_gemm(ra, q));
    }
    return 0;
}
// 3. reverse recurrence
static int bwd_recurrence(const BwdPlan& p, hipStream_t st) {
    const echr_dec_args* a = p.a; const echr_dec_grads* g = p.g; const DecWs& w = p.w; const DecWsBwd& b = p.b;
    if (p.bwd_persist) {
        // the whole reverse recurrence in two concurrent persistent launches (csrc/persist.hip)
        PersistBwdBufs pb;
        for (int k = 0; k < 3; ++k) { pb.GATES[k] = w.GATES[k]; pb.CS[k] = w.CS[k]; pb.DG[k] = b.DG[k]; }
        pb.QS = w.QS; pb.WT = w.WT; pb.ATT = w.ATT; pb.PALL = w.PALL; pb.DOUT = b.DOUT; pb.DQ = b.DQ; pb.DSC = b.DSC; pb.xws = b.XWSB;
        pb.prezeroed = (p.stages & BWD_HEAD) != 0;          // stage 1 of this call zeroed the exchange workspace with the backward scratch
        RC(persist_bwd(a, pb, p.dh, p.dout, st));
    } else {
        for (int t = p.S - 1; t >= 0; --t) RC(bwd_step(p, t, st));
    }
    if (a->h0 && g->g_h0) {          // d loss / d (initial state): what step 0 left in the d h accumulators + the carried d c
        const long n = (long)p.N * 3 * p.H;
        hipLaunchKernelGGL(init_state_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b.DHACC[0], b.DHACC[1], b.DHACC[2], b.DC, g->g_h0, p.N, p.H);
        RC(check_launch("init_state_grad"));
    }
    return 0;
}
// weight gradients that are sums over the S timesteps: W_hh_k, W_ih_k[:, :E], W_ih1[:, E:], W_h2a.
// beta = 0 writes, beta = 1 accumulates (p.zb).  HS[t] holds h(t-1), so rows t*N.. pair with DG[t].
static int bwd_weight_grads(const BwdPlan& p, hipStream_t q) {
    const echr_dec_grads* g = p.g; const DecWs& w = p.w; const DecWsBwd& b = p.b; const int H = p.H, E = p.E, Ha = p.Ha, D = p.D, SN = p.SN, SNr = p.SNr;
    if (p.h2) {
        // all S*N rows at once: DG_k^T, h(t-1)_k^T, XT^T, ATT^T, DQ^T packed (transposing) by one launch; DG_k^T is shared by the
        // W_hh, W_ih[:, :E] and W_ih1[:, E:] gradients, h1^T by the W_hh1 and W_h2a gradients
        H2PackJob pj[9];
        for (int k = 0; k < 3; ++k) {
            pj[k] = pack_cols(b.DG[k], 4 * H, 4 * H, SN, b.PK_DGT[k]);
            pj[3 + k] = pack_cols(w.HS + k * H, 3 * H, H, SN, b.PK_HT[k]);
        }
        pj[6] = pack_cols(w.XT, E, E, SN, b.PK_XTT);
        pj[7] = pack_cols(w.ATT, D, D, SN, b.PK_ATTT);
        pj[8] = pack_cols(b.DQ, Ha, Ha, SN, b.PK_DQT);
        if (p.crec)          // rows behind a caption's end carry d G = d q = 0 exactly: the contraction runs over the active rows only
            for (int i = 0; i < 9; ++i) { pj[i].K = SNr; pj[i].gather = p.actr; }
        RC(h2_pack_multi(pj, 9, q));
        // the seven products that contract d G_k^T over the S*N rows (W_hh x3, W_ih[:, :E] x3, W_ih1[:, E:]) share M = 4H and K, the W_h2a
        // gradient shares K: ONE grouped launch of 8 x 64 tile slots fills the chip in a single round (they were five launches)
        echr_gemm_desc g7[8];
        for (int k = 0; k < 3; ++k) {
            g7[k] = desc_h2(b.PK_DGT[k], b.PK_HT[k], g->g_w_hh[k], H, 4 * H, H, SNr);
            g7[3 + k] = desc_h2(b.PK_DGT[k], b.PK_XTT, g->g_w_ih[k], p.cin[k], 4 * H, E, SNr);
        }
        g7[6] = desc_h2(b.PK_DGT[1], b.PK_ATTT, g->g_w_ih[1] + E, p.cin[1], 4 * H, D, SNr);
        g7[7] = desc_h2(b.PK_DQT, b.PK_HT[1], g->g_w_h2a, H, Ha, H, SNr);      // d q^T . h1 (M = Ha): same K, rides along
        for (int i = 0; i < 8; ++i) g7[i].beta = p.zb;
        return gemm_grouped(g7, 8, q);
    }
    echr_gemm_desc e, ghh[3], gih[3];
    for (int k = 0; k < 3; ++k) {
        ghh[k] = desc_tn(b.DG[k], 4 * H, w.HS + k * H, 3 * H, g->g_w_hh[k], H, 4 * H, H, SN);
        ghh[k].beta = p.zb; ghh[k].split_k = -1;
        gih[k] = desc_tn(b.DG[k], 4 * H, w.XT, E, g->g_w_ih[k], p.cin[k], 4 * H, E, SN);
        gih[k].beta = p.zb; gih[k].split_k = -1;
    }
    RC(gemm_grouped(ghh, 3, q));        // three W_hh gradients in one launch
    RC(gemm_grouped(gih, 3, q));        // three W_ih[:, :E] gradients in one launch
    e = desc_tn(b.DG[1], 4 * H, w.ATT, D, g->g_w_ih[1] + E, p.cin[1], 4 * H, D, SN);
    e.beta = p.zb; e.split_k = -1;
    RC(gemm(e, q));
    e = desc_tn(b.DQ, Ha, w.HS + H, 3 * H, g->g_w_h2a, H, Ha, H, SN);
    e.beta = p.zb; e.split_k = -1;
    return gemm(e, q);
}
// bias gradients b_h2a and per stream b_ih = b_hh = column sums of DG_k over all S*N rows (stream 2's also as the plain vector DGCOL that the scene
// projection consumes).  One launch when the gradient buffers accumulate; the other form goes through the per-event sums DGSUM[0..2] and leaves them
static int bwd_bias_sums(const BwdPlan& p, hipStream_t q) {
    const echr_dec_grads* g = p.g; const DecWsBwd& b = p.b; const int N = p.N, S = p.S, H = p.H, Ha = p.Ha, SN = p.SN;
    if (p.z) {
        const ColsumJob cj[4] = {{b.DQ, Ha, SN, Ha, g->g_b_h2a, nullptr, nullptr},
                                 {b.DG[0], 4 * H, SN, 4 * H, g->g_b_ih[0], g->g_b_hh[0], nullptr},
                                 {b.DG[1], 4 * H, SN, 4 * H, g->g_b_ih[1], g->g_b_hh[1], nullptr},
                                 {b.DG[2], 4 * H, SN, 4 * H, g->g_b_ih[2], g->g_b_hh[2], b.DGCOL[2]}};
        return colsum_multi(cj, 4, q);
    }
    RC(colsum(b.DQ, Ha, SN, Ha, g->g_b_h2a, p.z, q));
    for (int k = 0; k < 3; ++k) {
        RC(sum_over_time(b.DG[k], 4 * H, S, N, 4 * H, b.DGSUM[k], 4 * H, q));
        RC(colsum2(b.DGSUM[k], 4 * H, N, 4 * H, g->g_b_ih[k], g->g_b_hh[k], p.z, q));       // b_ih and b_hh share their gradient
        if (k == 2) RC(colsum(b.DGSUM[k], 4 * H, N, 4 * H, b.DGCOL[k], false, q));          // also needed as a vector below
    }
    return 0;
}
// event context of stream 0, from d gates0 summed over time per event (`dgsum` [N, 4H]; EV_SUMS: formed here): the context half of W_ih0,
// d W_ih0[:, E:] = dgsum^T . event, and d event = dgsum . W_ih0[:, E:] (what the caller's next backward kernels, the event encoder's, wait for)
static int bwd_event_grads(const BwdPlan& p, int what, float* dgsum, hipStream_t q) {
    const echr_dec_args* a = p.a; const echr_dec_grads* g = p.g; const int N = p.N, H = p.H, E = p.E;
    if (what & EV_SUMS) RC(sum_over_time(p.b.DG[0], 4 * H, p.S, N, 4 * H, dgsum, 4 * H, q));
    echr_gemm_desc dw = desc_tn(dgsum, 4 * H, a->event, a->De, g->g_w_ih[0] + E, p.cin[0], 4 * H, a->De, N);
    dw.beta = p.zb; dw.split_k = -1;
    if (what & EV_D_WEIGHT) RC(gemm(dw, q));
    echr_gemm_desc de = desc_nn(dgsum, 4 * H, a->w_ih[0] + E, p.cin[0], g->g_event, a->De, N, a->De, 4 * H);
    de.split_k = -1; de.beta = 1.f;                                // zeroed with the backward scratch
    return (what & EV_D_EVENT) ? gemm(de, q) : 0;
}
// scene half of W_ih2 and d video.  One video: DGCOL[2] (column sum of d gates2) x the scene vector.  Multi-video batch: what stream 0's per-event
// context already does -- d gates2 summed over time per event (DGSUM[2]; have_sum: the caller has formed it), a segmented row sum by video in a fixed
// order (DGSEG [V, 4H]), then d W_ih2[:, E:] = DGSEG^T . video (K = V) and d video = DGSEG . W_ih2[:, E:], each one fixed-order k loop per tile
static int bwd_scene_grads(const BwdPlan& p, hipStream_t q, bool have_sum) {
    const echr_dec_args* a = p.a; const echr_dec_grads* g = p.g; const DecWsBwd& b = p.b; const int N = p.N, H = p.H, E = p.E;
    const echr_batch_ext* bx = p.c.bx;
    if (!bx) {
        RC(rank1_update(b.DGCOL[2], a->video, g->g_w_ih[2] + E, p.cin[2], 4 * H, a->Dv, false, q));          // K = 1: no GEMM launch
        if (g->g_video) RC(vec_mat(b.DGCOL[2], a->w_ih[2] + E, p.cin[2], g->g_video, 4 * H, a->Dv, q));
        return 0;
    }
    const int V = bx->n_videos;
    if (!have_sum) RC(sum_over_time(b.DG[2], 4 * H, p.S, N, 4 * H, b.DGSUM[2], 4 * H, q));
    float* dgseg = carve_batch(N, V, H, bx->ws).DGSEG;
    RC(seg_rowsum(b.DGSUM[2], bx->vid, N, V, 4 * H, 4 * H, dgseg, q));
    echr_gemm_desc ds = desc_tn(dgseg, 4 * H, bx->video, a->Dv, g->g_w_ih[2] + E, p.cin[2], 4 * H, a->Dv, V);
    ds.split_k = 1;
    RC(gemm(ds, q));
    if (!bx->g_video) return 0;
    ds = desc_nn(dgseg, 4 * H, a->w_ih[2] + E, p.cin[2], bx->g_video, a->Dv, V, a->Dv, 4 * H);
    ds.split_k = 1;
    return gemm(ds, q);
}
// token embedding: dXT = sum_k DG_k . W_ih_k[:, :E], scatter-added into the (caller-zeroed) table gradient.  Reads what the recurrence left (DG) and
// parameters only, so the chain rides on the prepare stream behind the LSTM-layer stage: the three streams of the backward tail end together
static int bwd_embed_grads(const BwdPlan& p, hipStream_t q) {
    const echr_dec_args* a = p.a; const DecWsBwd& b = p.b; const int H = p.H, E = p.E, SN = p.SN, SNr = p.SNr;
    echr_gemm_desc gx[3];
    if (p.h2) {
        H2PackJob pj[6];
        for (int k = 0; k < 3; ++k) {
            pj[k] = pack_rows(b.DG[k], 4 * H, SNr, 4 * H, b.PK_DG[k]);
            pj[k].gather = p.actr;          // (compact: d XT is formed for the active rows only, row i of it belongs to position act[i])
            pj[3 + k] = pack_cols(a->w_ih[k], p.cin[k], E, 4 * H, b.PK_WIHT[k]);
        }
        RC(h2_pack_multi(pj, 6, q));
    }
    // dXT is materialised, not added by the products' epilogues straight into the table gradient row of its token (echr_gemm_desc.row_index):
    // measured on one box, alternating runs, 1.74 ms per iteration against 1.94 -- every k-slice of every product would send its atomics to the
    // table, and the 64 <bos> rows of a batch (plus frequent words) serialise on the same addresses; the dense d XT buffer takes the k-slice
    // atomics without contention and the scatter pass meets each duplicate once (20 us, `tools/skip_bounds.py`)
    for (int k = 0; k < 3; ++k) {
        gx[k] = p.h2 ? desc_h2(b.PK_DG[k], b.PK_WIHT[k], b.DXT, E, SNr, E, 4 * H) : desc_nn(b.DG[k], 4 * H, a->w_ih[k], p.cin[k], b.DXT, E, SN, E, 4 * H);
        gx[k].split_k = -1; gx[k].beta = 1.f;                // shared, pre-zeroed output: everything adds atomically
    }
    // (a grouped launch whose problems share C adds its k-slices atomically and needs two of them: K = 4H <= 32, i.e. H = 4 or 8, runs the
    // three accumulating products one behind the other instead, as tsrm.hip does for d X)
    if (4 * H > 32) RC(gemm_grouped(gx, 3, q));
    else for (int k = 0; k < 3; ++k) RC(gemm(gx[k], q));
    return embed_scatter_add(b.DXT, a->tokens, p.g->g_embed, p.h2 ? SNr : SN, E, p.V1, q, p.h2 ? p.actr : nullptr);
}
// 5. attention parameters: d P_all / d alpha over all timesteps (att_post), the column sums behind it (bias_owed: with d b_logit) and ctx2att
static int bwd_attention_params(const BwdPlan& p, bool bias_owed, hipStream_t st) {
    const echr_dec_args* a = p.a; const echr_dec_grads* g = p.g; const DecWs& w = p.w; const DecWsBwd& b = p.b; const int N = p.N, S = p.S, Ha = p.Ha, A = p.A, D = p.D;
    const bool z = p.z;
    const double fl = 6.0 * N * A * Ha * S, by = 4.0 * ((double)N * A * Ha * 2 + (double)S * N * (Ha + A));
    const AttDims ad{N, A, Ha, D};
    if (det_mode()) {          // fixed-order mode: the profile scope spans the fixed-order column sums too
        ProfScope prof(PROF_ATT_POST, fl, by, st);
        float *ga, *gb; int nblk;
        RC(att_post_fixed_order(ad, a->Tv, S, a->rows_disjoint, w.PALL, w.QS, a->w_alpha, b.DSC, a->ev_start, a->ev_len, b.DPALL, &ga, &gb, &nblk, st));
        RC(colsum(ga, Ha, nblk, Ha, g->g_w_alpha, z, st));
        RC(colsum(gb, 1, nblk, 1, g->g_b_alpha, z, st));
        if (z) {
            RC(colsum(b.DPALL, Ha, a->Tv, Ha, g->g_b_c2a, z, st));
            if (bias_owed) RC(colsum(b.DLG, b.ldg, p.SNc, p.V1, g->g_b_logit, z, st));
        }
    } else {
        { ProfScope prof(PROF_ATT_POST, fl, by, st);
          RC(launch_att_post(ad, w.PALL, w.QS, a->w_alpha, b.DSC, a->ev_start, a->ev_len, b.DPALL, b.GAREP, b.GBREP, S, a->rows_disjoint ? 1 : 0, st)); }
        if (z) {
            // accumulate mode: the replicas -> d alpha, d b_alpha, the ctx2att bias gradient (column sums of d P_all) and -- when the logit-layer
            // gradients were formed on this stream just before -- d b_logit: ONE multi-problem launch instead of four
            ColsumJob sums[4] = {{b.GAREP, Ha, ALPHA_REP, Ha, g->g_w_alpha, nullptr, nullptr}, {b.GBREP, 1, ALPHA_REP, 1, g->g_b_alpha, nullptr, nullptr},
                                 {b.DPALL, Ha, a->Tv, Ha, g->g_b_c2a, nullptr, nullptr}, {b.DLG, b.ldg, p.SNc, p.V1, g->g_b_logit, nullptr, nullptr}};
            RC(colsum_multi(sums, bias_owed ? 4 : 3, st));
        } else {
            RC(colsum(b.GAREP, Ha, ALPHA_REP, Ha, g->g_w_alpha, z, st));        // replicas -> d alpha, d b_alpha (overwrite or accumulate like every
            RC(colsum(b.GBREP, 1, ALPHA_REP, 1, g->g_b_alpha, z, st));          // other parameter gradient)
        }
    }
    echr_gemm_desc d;
    if (p.h2) {
        H2PackJob pj[2] = {pack_cols(b.DPALL, Ha, Ha, a->Tv, b.PK_DPT), pack_cols(a->c3d, D, D, a->Tv, b.PK_C3DT)};
        RC(h2_pack_multi(pj, 2, st));
        d = desc_h2(b.PK_DPT, b.PK_C3DT, g->g_w_c2a, D, Ha, D, a->Tv);
    } else {
        d = desc_tn(b.DPALL, Ha, a->c3d, D, g->g_w_c2a, D, Ha, D, a->Tv);
        d.split_k = -1;
    }
    d.beta = p.zb;
    RC(gemm(d, st));
    return z ? 0 : colsum(b.DPALL, Ha, a->Tv, Ha, g->g_b_c2a, z, st);
}
// the LSTM-layer gradients behind the recurrence on one stream: weight gradients, bias sums, event context (`ev`: EV_*), scene gradients
static int bwd_lstm_grads(const BwdPlan& p, int ev, float* dgsum0, hipStream_t q) {
    RC(bwd_weight_grads(p, q));
    RC(bwd_bias_sums(p, q));
    RC(bwd_event_grads(p, ev, dgsum0, q));
    return bwd_scene_grads(p, q, !p.z);          // (the non-accumulating bias form has formed every stream's per-event sums)
}
// 4. batched parameter gradients of the three LSTM layers (core.layer0..2) -- final after this stage, so a data-parallel caller can start reducing
//    them (phase 3) while the tail stage runs.  Three schedules: the caller's stream, accumulating (the per-event sums of stream 0 feed the
//    event-context products) or not, and async_tail = 2: only d event (what the caller's next backward kernels, the event encoder's, wait for) is
//    formed on the caller's stream, first; the rest -- nine transposing packs, the grouped weight-gradient product, bias sums, the context halves
//    of W_ih: ~0.13 ms -- moves to the prepare stream (idle during a backward pass) and is joined by echr_stream_join like the tail
static int bwd_lstm_stage(const BwdPlan& p, hipStream_t st, BwdSched& s) {
    float* const* dgsum = p.b.DGSUM;
    if (!(p.stages & BWD_LSTM)) return 0;
    if (!p.lstm_on_helper) return bwd_lstm_grads(p, (p.z ? EV_SUMS : 0) | EV_D_WEIGHT | EV_D_EVENT, dgsum[0], st);
    // Both helper streams fork RIGHT BEHIND the reverse recurrence, off ONE recorded event, not behind d event with one record each: the
    // two records used to sit between the d event product and everything that follows on all three streams (~15 us of an idle chip).
    // The prepare stream then forms its own copy of the per-event gate-gradient sums (6 us) instead of waiting for this stream's
    const bool whole = p.part == 0;
    const hipStream_t early = whole ? aux2_fork(st) : nullptr;
    if (early) fork_event(prep().fork);          // the tail stage's fork waits for the same event
    if (p.part != 2) RC(bwd_event_grads(p, EV_SUMS | EV_D_EVENT, dgsum[0], st));
    if (p.part == 1) return 0;
    const hipStream_t q = whole ? early : aux2_fork(st);
    if (!q) return bwd_lstm_grads(p, EV_D_WEIGHT, dgsum[0], st);          // (no second helper stream: the rest follows d event on the caller's stream)
    if (whole) RC(bwd_event_grads(p, EV_SUMS, dgsum[1], q));
    RC(bwd_lstm_grads(p, EV_D_WEIGHT, dgsum[whole ? 1 : 0], q));
    RC(handover_mark(p.c, ECHR_HANDOVER_LSTM, q));          // every gradient of core.layer0..2 is final here
    if (p.stages & BWD_TAIL) { RC(bwd_embed_grads(p, q)); s.embed_queued = true; }
    if (hipEventRecord(tail().done3, q) != hipSuccess) { set_error("decoder_bwd: event record failed"); return -5; }
    tail().pending3 = true;
    return 0;
}
// the tail: deferred logit-layer gradients, attention parameters, token embedding (unless the prepare stream took it).  phase 0 + async_tail: nothing
// downstream in the backward pass needs its outputs -> the tail stream, joined by the caller.  Its three chains read only what the recurrence left
// (DLG, OUTD, DG, DQ, DSC); the tail forks behind the LSTM-layer stage, not ahead of it: measured on one box, alternating runs, 1.726 vs 1.731 ms
// per iteration -- this phase is bound by its chip-filling GEMMs, packs and att_post (~0.4 ms), not by stream order
static int bwd_tail_stage(const BwdPlan& p, hipStream_t sm, BwdSched& s) {
    if (!(p.stages & BWD_TAIL)) return 0;
    const hipStream_t st = p.async_tail ? tail().s : sm;
    if (p.async_tail) {
        if (hipEvent_t fe = fork_event_slot()) {          // (forked with the prepare stream, right behind the reverse recurrence)
            if (hipStreamWaitEvent(st, fe, 0) != hipSuccess) { set_error("decoder_bwd: stream fork failed"); return -5; }
        } else RC(hop(sm, tail().fork, st));
        RC(bwd_logit_grads_on_tail(p, st, s));
    }
    RC(bwd_attention_params(p, s.bias_owed, st));
    if (!s.embed_queued) RC(bwd_embed_grads(p, st));
    if (p.async_tail) {
        if (hipEventRecord(tail().done, st) != hipSuccess) { set_error("decoder_bwd: event record failed"); return -5; }
        tail().pending = true;
    }
    return 0;
}
static int bwd_stages(const BwdPlan& p, hipStream_t st) {
    BwdSched s;
    if (p.stages & BWD_HEAD) { RC(bwd_dlogits_and_scratch(p, st)); RC(bwd_late_fusion(p, st)); }
    if (p.stages & BWD_REC) RC(bwd_recurrence(p, st));
    RC(bwd_lstm_stage(p, st, s));
    return bwd_tail_stage(p, st, s);
}
int echr::decoder_bwd_parts(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream, int part, const DecCall& c) {
    if (prep().fill_pending) {          // (a stream wait, not a launch: the caller's arena fill is ordered in front of whatever follows, refused or not)
        prep().fill_pending = false;
        if (hipStreamWaitEvent((hipStream_t)stream, prep().fill_done, 0) != hipSuccess) { set_error("decoder_bwd: stream wait failed"); return -5; }
    }
    BwdPlan p;
    RC(bwd_plan(a, g, drop, part, c, p));
    const int rc = bwd_stages(p, (hipStream_t)stream);
    fork_event(nullptr);
    return rc;
}

// ------------------------------------------------------------------------------------------------------
// greedy sampler (OldModel_NEW.py:139-187, sample_max = 1, eval mode): every step on device
// ------------------------------------------------------------------------------------------------------
struct SampWs { float* XT; float* LOGITS; int *IT, *UNF; float* SLABS; float *TABLES, *PSWS, *PSX;
                // many events, launch-per-step form: h2 images of the recurrent weights (packed once per decode) and of the step's h / context rows
                float *PK_WHH[3], *PK_WH2A, *PK_WATT, *PK_H[3], *PK_ATT; long total; };
// parameter-only operands of the persistent greedy decoder (csrc/persist.hip, PersistS): the token-side gate tables, the packed embedding
// they are made from and the logit-weight image -- cacheable across calls while the parameters do not change (echr_sample_args.tables)
struct SampTables { float *TG[3], *PK_EMB, *LIMG; long total; };
static SampTables carve_tables(const echr_dec_args* a, float* base) {
    SampTables s;
    long off = 0;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += rup(n, 64); return p; };
    for (int k = 0; k < 3; ++k) s.TG[k] = take((long)a->V1 * 4 * a->H);
    s.PK_EMB = take(h2_floats(a->V1, a->E));
    s.LIMG = take(persist_logit_image_floats(a->V1));
    s.total = off;
    return s;
}
// few events (N < SAMP_SLAB_ROWS): one k loop per tile of the per-step logits product would be 48 k blocks deep on 79 workgroups; its K is cut into
// SAMP_SLABS slices that run as a strided batch into slabs (plain stores), and the arg-max kernel adds the slabs in a fixed order (bitwise
// reproducible).  Measured alternatives at N = 64 (1 GF, 30.7 MB of weights per step): 8 slices 20 us, 12 slices on the recurrence's grouped
// skinny-GEMM kernel 21 us, 4 slices 23 us -- the product sits at the fp32-MFMA + weight-streaming floor of ~15 us either way; 4 slices write
// the fewest slab bytes
constexpr int SAMP_SLAB_ROWS = 192;
constexpr int SAMP_SLABS = 4;
static inline int samp_slabs(const echr_dec_args* a) { (void)a; return SAMP_SLABS; }
static SampWs carve_samp(const echr_dec_args* a, float* base, bool persist_bufs = true) {
    SampWs s;
    long off = 0;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += rup(n, 64); return p; };
    s.XT = take((long)a->N * a->E);
    s.LOGITS = take((long)a->N * a->V1);
    s.IT = reinterpret_cast<int*>(take(a->N));
    s.UNF = reinterpret_cast<int*>(take(a->N));
    s.SLABS = take(a->N < SAMP_SLAB_ROWS ? (long)((samp_slabs(a) + 3) / 4 * 4) * a->N * a->V1 : 64);
    // persistent decoding (csrc/persist.hip, PersistS): token-side gate tables, the packed embedding they are made from, the logit-weight
    // image and the launch's exchange buffers
    const bool ps = persist_bufs && persist_sample_shape_ok(a);          // by shape only: the carving must not depend on switches that can change between calls
    s.TABLES = take(ps ? carve_tables(a, nullptr).total : 64);
    const long groups = (a->N + 63) / 64;          // the persistent decoder runs one launch per group of 64 events, each on its own workspaces
    s.PSWS = take(ps ? groups * persist_sample_ws_floats(a->S, a->V1) : 64);
    s.PSX = take(ps ? groups * persist_sample_x_floats(a->S) : 64);
    const bool bigw = a->N >= SAMP_SLAB_ROWS;          // (by shape only)
    for (int k = 0; k < 3; ++k) s.PK_WHH[k] = take(bigw ? h2_floats(4 * a->H, a->H) : 64);
    s.PK_WH2A = take(bigw ? h2_floats(a->Ha, a->H) : 64);
    s.PK_WATT = take(bigw ? h2_floats(4 * a->H, a->D) : 64);
    for (int k = 0; k < 3; ++k) s.PK_H[k] = take(bigw ? h2_floats(a->N, a->H) : 64);
    s.PK_ATT = take(bigw ? h2_floats(a->N, a->D) : 64);
    s.total = off;
    return s;
}
// which form echr_decoder_sample takes for greedy decoding: the persistent launches (one per 64 events: latency-optimal, 22 us per step and
// group) up to "persist_sample_max" events, beyond that -- evaluation over hundreds of proposals -- one batched launch chain per step
// whose products all run as h2 GEMMs over the N rows (throughput-optimal: the 16 groups of N = 1000 would queue up behind each other)
static bool sample_uses_persistent(const echr_dec_args* a) {
    if (!persist_sample_eligible(a)) return false;
    const int mx = config().persist_sample_max;
    return !(config().gemm_h2 && mx > 0 && a->N > mx && a->N >= SAMP_SLAB_ROWS);
}

// One decoder timestep over MANY events (evaluation: hundreds of proposals; launch-per-step greedy decoding).  step_fwd's grouped skinny
// products are built for N <= 64 rows (K split over workgroups, fp32 MFMA: 94 us per launch at N = 1000); here every product is an h2 GEMM over
// the N rows with ONE fixed-order k loop per tile (bitwise reproducible): GATES[k][t] (which holds the token-side pre-activations) += h_k(t-1) .
// W_hh_k^T and q(t) += h1(t-1) . W_h2a^T (its own zero-filled slab) as one grouped launch, then the attention kernels, then GATES[1][t] += ctx . W_ih1[:, E:]^T.
static int step_fwd_big(const echr_dec_args* a, const DecWs& w, const SampWs& s, int t, const DropCfg& dh, const DropCfg& dout, hipStream_t st) {
    const int N = a->N, H = a->H, Ha = a->Ha, A = a->A, D = a->D;
    const float* hprev = w.HS + (long)t * N * 3 * H;          // [N,3H] h of step t-1 (zeros at t = 0)
    const long gs = (long)N * 4 * H, qs = (long)N * Ha;
    (void)hprev;
    float* qt = w.QACC + (long)t * qs;          // this step's q: its own zero-filled slab (the caller cleared QACC once), so the product accumulates
    if (t > 0 || a->h0) {          // (h(-1) = 0 without echr_dec_args.h0: nothing to add at the first step; q = 0 then, the score kernel adds b_h2a)
        echr_gemm_desc g4[4];          // the caller packed h(t-1) of the three streams with the step's token embeddings
        for (int k = 0; k < 3; ++k) g4[k] = desc_h2(s.PK_H[k], s.PK_WHH[k], w.GATES[k] + (long)t * gs, 4 * H, N, 4 * H, H);
        g4[3] = desc_h2(s.PK_H[1], s.PK_WH2A, qt, Ha, N, Ha, H);
        for (int i = 0; i < 4; ++i) { g4[i].beta = 1.f; g4[i].split_k = 1; }
        RC(gemm_grouped(g4, 4, st));
    }
    float* q = w.QS + (long)t * N * Ha;
    float* sc = w.SC + (long)t * N * A;
    float* wt = w.WT + (long)t * N * A;
    float* att = w.ATT + (long)t * N * D;
    {
        const double rows = (double)N * A;
        ProfScope prof(PROF_ATT_FWD, 2.0 * rows * (Ha + D), 4.0 * (rows * (Ha + D + 2) + (double)N * (Ha + D)), st);
        const AttDims ad{N, A, Ha, D};
        RC(launch_att_score(ad, w.PALL, qt, 1, qs, a->b_h2a, q, a->w_alpha, a->b_alpha, a->ev_start, a->ev_len, sc, st));
        hipLaunchKernelGGL(att_context_kernel, dim3(N, (D + 127) / 128), dim3(256), (((A + 31) & ~31) + 8 * 128) * sizeof(float), st, a->c3d, sc,
                           a->ev_start, a->ev_len, wt, att, A, D);
        RC(check_launch("att_context"));
    }
    {
        H2PackJob pj = pack_rows(att, D, N, D, s.PK_ATT);
        RC(h2_pack_multi(&pj, 1, st));
        echr_gemm_desc d = desc_h2(s.PK_ATT, s.PK_WATT, w.GATES[1] + (long)t * gs, 4 * H, N, 4 * H, D);
        d.beta = 1.f; d.split_k = 1;
        RC(gemm(d, st));
    }
    LstmPtrs P;
    for (int k = 0; k < 3; ++k) {
        P.gates[k] = w.GATES[k] + (long)t * gs;
        P.slab[k] = w.GSL[k];
        P.nslab[k] = 0;
        P.base[k] = nullptr; P.base2[k] = nullptr; P.bmod[k] = 1;
        P.c_prev[k] = w.CS[k] + (long)t * N * H;
        P.c_new[k] = w.CS[k] + (long)(t + 1) * N * H;
        P.kmap[k] = k;
    }
    P.slab_stride = gs;
    hipLaunchKernelGGL(lstm_pointwise_fwd_kernel, dim3((N * H + 255) / 256, 3), dim3(256), 0, st, P,
                       w.HS + (long)(t + 1) * N * 3 * H, w.OUTD + (long)t * N * 3 * H, N, H, t, dh, dout);
    return check_launch("lstm_pointwise_fwd");
}

// LOGITS = (...((S0 + S1) + (S2 + S3)) + ((S4 + S5) + (S6 + S7)) ...) + bias: the k-slices of the logits product in groups of four, one fixed
// order (bitwise reproducible, unlike atomics); nslab is a multiple of 4 (spare slabs are zero)
__global__ __launch_bounds__(256) void slab_sum_bias_kernel(const float* __restrict__ slabs, long slab_stride, int nslab, const float* __restrict__ bias,
                                                            float* __restrict__ out, long n, int V1) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int s0 = 0; s0 < nslab; s0 += 4) {
        const float* sp = slabs + (long)s0 * slab_stride + i;
        const float part = (sp[0] + sp[slab_stride]) + (sp[2 * slab_stride] + sp[3 * slab_stride]);
        v = s0 == 0 ? part : v + part;
    }
    out[i] = v + (bias ? bias[i % V1] : 0.f);
}
extern "C" int64_t echr_sampler_ws_floats(const echr_dec_args* a) { return a ? carve_samp(a, nullptr).total : -1; }
extern "C" int64_t echr_sampler_table_floats(const echr_dec_args* a) {
    if (!a) return -1;
    return sample_uses_persistent(a) ? carve_tables(a, nullptr).total : 0;
}

// The launch-per-step decode chain shared by the sampler (decoder_sample_impl) and beam search (echr_decoder_beam).  chain_setup runs
// once per decode, chain_step once per step: the decoder timestep from IT (the tokens fed at step t) and the logits product.  `big`
// (many rows with gemm_h2: every product an h2 GEMM over the rows) is decided by the caller once per decode.  With the slab form of the
// logits product (few rows) the logits are left as k-slice slabs in SLABS unless `sum_slabs` asks for them in LOGITS (*slab_form says
// which); otherwise LOGITS holds them, bias included.
static int chain_setup(const echr_dec_args& a, const DecWs& w, const SampWs& s, bool big, hipStream_t st) {
    const int N = a.N, H = a.H, E = a.E, L = a.S;
    RC(precompute_static(&a, w, st, big));
    if (big) RC(fill_zero(w.QACC, (long)L * N * a.Ha, st));          // q(t) slabs of step_fwd_big
    if (big) {          // recurrent weights as h2 operands, once per decode
        H2PackJob pj[5] = {pack_rows(a.w_hh[0], H, 4 * H, H, s.PK_WHH[0]), pack_rows(a.w_hh[1], H, 4 * H, H, s.PK_WHH[1]),
                           pack_rows(a.w_hh[2], H, 4 * H, H, s.PK_WHH[2]), pack_rows(a.w_h2a, H, a.Ha, H, s.PK_WH2A),
                           pack_rows(a.w_ih[1] + E, E + a.D, 4 * H, a.D, s.PK_WATT)};
        RC(h2_pack_multi(pj, 5, st));
    }
    const int nsl = samp_slabs(&a), nsl4 = (nsl + 3) / 4 * 4;          // slabs are added four at a time: the spare ones stay zero
    if (N < SAMP_SLAB_ROWS && nsl4 > nsl) RC(fill_zero(s.SLABS + (long)nsl * N * a.V1, (long)(nsl4 - nsl) * N * a.V1, st));
    return 0;
}
static int chain_step(const echr_dec_args& a, const DecWs& w, const SampWs& s, int t, bool big, const DropCfg& dh, const DropCfg& dout,
                      bool sum_slabs, bool* slab_form, hipStream_t st) {
    const int N = a.N, H = a.H, E = a.E;
    const int nsl4 = (samp_slabs(&a) + 3) / 4 * 4;
    if (big) {
        RC(embed_gather(a.embed, s.IT, s.XT, N, E, a.V1, st));
        {   // the step's h2 operands in ONE pack launch: the token embeddings and the three streams' h(t-1)
            const float* hprev = w.HS + (long)t * N * 3 * H;
            H2PackJob pj[4] = {pack_rows(s.XT, E, N, E, w.PK_XT), pack_rows(hprev, 3 * H, N, H, s.PK_H[0]), pack_rows(hprev + H, 3 * H, N, H, s.PK_H[1]),
                               pack_rows(hprev + 2 * H, 3 * H, N, H, s.PK_H[2])};
            RC(h2_pack_multi(pj, (t > 0 || a.h0) ? 4 : 1, st));
        }
        RC(input_gates(&a, w, s.XT, t, 1, st, false, true, true));
        RC(step_fwd_big(&a, w, s, t, dh, dout, st));
    } else {
        // few events: no embedding gather, no input-gate GEMM -- the token-side products are jobs of the step's first grouped launch
        // (rows gathered from the embedding table by token id), the time-invariant addends are read by the gate kernel
        RC(step_fwd(&a, w, t, dh, dout, st, false, s.IT));
    }
    *slab_form = false;
    if (big) {
        H2PackJob pj = pack_rows(w.OUTD + (long)t * N * 3 * H, 3 * H, N, 3 * H, w.PK_OUTD);
        RC(h2_pack_multi(&pj, 1, st));
        echr_gemm_desc d = desc_h2(w.PK_OUTD, w.PK_WL, s.LOGITS, a.V1, N, a.V1, 3 * H);
        d.bias = a.b_logit; d.split_k = 1;
        RC(gemm(d, st));
    } else if (N < SAMP_SLAB_ROWS && (3 * H) % (SAMP_SLABS * 32) == 0) {
        const int ksl = 3 * H / SAMP_SLABS;
        echr_gemm_desc d = desc_nt(w.OUTD + (long)t * N * 3 * H, 3 * H, a.w_logit, 3 * H, s.SLABS, a.V1, N, a.V1, ksl);
        d.batch = SAMP_SLABS; d.bsa = ksl; d.bsb = ksl; d.bsc = (long)N * a.V1; d.split_k = 1;
        RC(gemm(d, st));
        *slab_form = true;
        if (sum_slabs) {         // the multinomial / beam steps read finished logits: sum the slabs first (the greedy step folds the sum in)
            const long n = (long)N * a.V1;
            hipLaunchKernelGGL(slab_sum_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s.SLABS, n, nsl4, a.b_logit, s.LOGITS, n, a.V1);
            RC(check_launch("slab_sum_bias"));
        }
    } else {
        echr_gemm_desc d = desc_nt(w.OUTD + (long)t * N * 3 * H, 3 * H, a.w_logit, 3 * H, s.LOGITS, a.V1, N, a.V1, 3 * H);
        d.bias = a.b_logit; d.split_k = 1;
        RC(gemm(d, st));
    }
    return 0;
}

// drop != nullptr: echr_decoder_sample_train -- the launch-per-step chain with the caller's training-mode dropout masks, keyed like
// echr_decoder_fwd's step t: (element, t, site, drop->offset)
// row_step: the multinomial step as ONE launch that forms the row from the slabs and draws (sample_row_step; the batched training decode)
// c: the call's batch extension and scene_rows (DecCall; the criterion weight and the hand-over are not read here)
static int decoder_sample_impl(const echr_sample_args* sa, const echr_dropout* drop, void* stream, const DecCall& c, bool row_step = false);
extern "C" int echr_decoder_sample(const echr_sample_args* sa, void* stream) { return decoder_sample_impl(sa, nullptr, stream, DecCall{}); }
extern "C" int echr_decoder_sample_train(const echr_sample_args* sa, const echr_dropout* drop, void* stream) {
    ECHR_REQUIRE(sa && drop, "decoder_sample_train: null args");
    ECHR_REQUIRE(sa->multinomial, "decoder_sample_train: the training-mode decode is the multinomial one (multinomial = 1)");
    return decoder_sample_impl(sa, drop, stream, DecCall{});
}
extern "C" int echr_decoder_sample_batch(const echr_sample_args* sa, const echr_batch_ext* x, void* stream) {
    ECHR_REQUIRE(sa && !sa->multinomial, "decoder_sample_batch: the batched decode is the greedy one (multinomial = 0)");
    RC(check_batch(&sa->dec, x, "decoder_sample_batch"));
    return decoder_sample_impl(sa, nullptr, stream, dec_batch_call(x));
}
// The sampled pass of self-critical training over a multi-video batch: echr_decoder_sample_train with the per-row scene part formed as each
// video's own call forms it (scene_rows), the multinomial step as one launch per step, and the per-video widths behind the last step on the same stream
extern "C" int echr_decoder_sample_train_batch(const echr_sample_args* sa, const echr_dropout* drop, const echr_batch_ext* x, int32_t* video_words,
                                               void* stream) {
    ECHR_REQUIRE(sa && drop && video_words, "decoder_sample_train_batch: null args / video_words");
    ECHR_REQUIRE(sa->multinomial, "decoder_sample_train_batch: the training-mode decode is the multinomial one (multinomial = 1)");
    RC(check_batch(&sa->dec, x, "decoder_sample_train_batch"));
    ECHR_REQUIRE(x->n_videos <= 65535, "decoder_sample_train_batch: at most 65535 videos per call (got %d)", x->n_videos);
    RC(decoder_sample_impl(sa, drop, stream, dec_batch_call(x, true), true));
    return sample_video_words(reinterpret_cast<const long long*>(sa->seq), x->vid, sa->dec.N, sa->seq_len, x->n_videos, video_words,
                              (hipStream_t)stream);
}
static int decoder_sample_impl(const echr_sample_args* sa, const echr_dropout* drop, void* stream, const DecCall& c, bool row_step) {
    ECHR_REQUIRE(sa, "decoder_sample: null args");
    RC(persist_check_async());
    DeterministicScope det;                    // `seq` is an index output: bitwise reproducible logits (no atomic split-K anywhere below)
    echr_dec_args a = sa->dec;
    const int L = sa->seq_len;
    ECHR_REQUIRE(L > 0 && sa->seq && sa->seq_logp && sa->n_unfinished && sa->ws_sample && a.ws, "decoder_sample: missing buffers");
    a.S = L;                                   // workspace is carved for seq_len steps
    RC(check_dims(&a, "decoder_sample"));
    hipStream_t st = (hipStream_t)stream;
    const int N = a.N, H = a.H, E = a.E;
    DecWs w = carve_ws(&a, a.ws, c.bx, c.scene_rows);
    SampWs s = carve_samp(&a, sa->ws_sample);
    const DropCfg dh = make_drop(drop, drop ? drop->p_h : 0.f), dout = make_drop(drop, drop ? drop->p_out : 0.f);          // (nullptr: identity)
    const bool persistent = !sa->multinomial && !drop && sample_uses_persistent(&a);
    {
        // one fill launch: the launch-per-step form starts from zero state / <bos> = 0 and zero outputs; the persistent form writes every
        // output element itself and only needs the unfinished counters cleared
        float* zp[8] = {reinterpret_cast<float*>(sa->n_unfinished), w.HS, w.CS[0], w.CS[1], w.CS[2], reinterpret_cast<float*>(s.IT),
                        reinterpret_cast<float*>(sa->seq), sa->seq_logp};
        long zn[8] = {L + 1, (long)N * 3 * H, (long)N * H, (long)N * H, (long)N * H, N, 2L * N * L, (long)N * L};
        RC(fill_zero_multi(zp, zn, persistent ? 1 : 8, st));
    }
    if (a.h0 && !persistent) RC(init_state_copy(&a, w, st));          // OldModel.sample starts from init_hidden too (:141)
    // many events (evaluation: up to 1000 proposals): the per-step token-side gate products and the logits product are 6 + 15 GF -- they run
    // on h2 operands (weights packed once per decode, the step's N rows packed per step; one fixed-order k loop per tile, so the decode stays
    // bitwise reproducible).  Few events: exact fp32 MFMA as before (the products are launch-bound there).
    if (persistent) {
        // every step on device: one persistent launch per 64 events.  Per call: the time-invariant products, the token-side gate tables
        // TG_k = embed . W_ih_k[:, :E]^T (+ the stream's biases / video part; the event part of stream 0 stays per event) and the logit image
        // TG_k = embed . W_ih_k[:, :E]^T (+ stream 1's biases; the event part of stream 0 and the video part of stream 2 stay outside: they
        // are inputs, not parameters) and the logit image: rebuilt unless the caller's cache is valid
        const SampTables tb = carve_tables(&a, sa->tables ? sa->tables : s.TABLES);
        const bool rebuild = !(sa->tables && sa->tables_valid);
        RC(precompute_static(&a, w, st, rebuild));
        if (rebuild) {
            H2PackJob pj = pack_rows(a.embed, E, a.V1, E, tb.PK_EMB);
            RC(h2_pack_multi(&pj, 1, st));
            echr_gemm_desc d[3];
            for (int k = 0; k < 3; ++k) {
                d[k] = desc_h2(tb.PK_EMB, w.PK_WIH[k], tb.TG[k], 4 * H, a.V1, 4 * H, E);
                d[k].split_k = 1;
                if (k == 1) { d[k].bias = a.b_ih[1]; d[k].bias2 = a.b_hh[1]; }
            }
            RC(gemm_grouped(d, 3, st));
            RC(persist_logit_image(a.w_logit, a.V1, tb.LIMG, st));
        }
        PersistSampleBufs B;
        B.PALL = w.PALL; B.EVB0 = w.EVB0; B.VIDB = w.scene; B.xws = s.PSX;
        B.vidb_ld = w.scene_ld;          // multi-video batch: the scene part of stream 2 is per event
        for (int k = 0; k < 3; ++k) B.TG[k] = tb.TG[k];
        B.limg = tb.LIMG; B.sws = s.PSWS;
        B.seq = reinterpret_cast<long long*>(sa->seq); B.seq_logp = sa->seq_logp; B.n_unfinished = sa->n_unfinished;
        RC(persist_sample(&a, B, st));
        return 0;
    }
    const bool big = config().gemm_h2 && N >= SAMP_SLAB_ROWS;
    RC(chain_setup(a, w, s, big, st));
    const int nsl4 = (samp_slabs(&a) + 3) / 4 * 4;
    for (int t = 0; t < L; ++t) {
        bool slab_form = false;
        RC(chain_step(a, w, s, t, big, dh, dout, sa->multinomial != 0 && !row_step, &slab_form, st));
        if (sa->multinomial && row_step)
            RC(sample_row_step(s.LOGITS, a.V1, N, a.V1, t, L, s.IT, s.UNF, reinterpret_cast<long long*>(sa->seq), sa->seq_logp, sa->n_unfinished,
                               sa->temperature, sa->seed, st, slab_form ? s.SLABS : nullptr, (long)N * a.V1, a.b_logit, nsl4));
        else if (sa->multinomial)
            RC(sample_step(s.LOGITS, a.V1, N, a.V1, t, L, s.IT, s.UNF, reinterpret_cast<long long*>(sa->seq), sa->seq_logp, sa->n_unfinished,
                           sa->temperature, sa->seed, st));
        else
            RC(greedy_step(s.LOGITS, a.V1, N, a.V1, t, L, s.IT, s.UNF, reinterpret_cast<long long*>(sa->seq), sa->seq_logp,
                           sa->n_unfinished, st, slab_form ? s.SLABS : nullptr, (long)N * a.V1, a.b_logit, nsl4));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// beam search (echr_decoder_beam): the launch-per-step chain over events * B rows, one beam_step launch per step (beam.hip)
// ------------------------------------------------------------------------------------------------------
struct BeamWs { SampWs s; BeamState b; long total; };
static BeamWs carve_beam(const echr_dec_args* a, int B, float* base) {          // a->N = rows, a->S = seq_len
    BeamWs r;
    r.s = carve_samp(a, base, false);          // (never the persistent decoder)
    long off = r.s.total;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += rup(n, 64); return p; };
    const long N = a->N, E = N / B, L = a->S;
    r.b.SCORE = take(N);
    r.b.ALIVE = reinterpret_cast<int*>(take(N));
    r.b.HTOK = reinterpret_cast<int*>(take(N * L));
    r.b.HLP = take(N * L);
    r.b.BTOK = reinterpret_cast<int*>(take(E * L));
    r.b.BLP = take(E * L);
    r.b.BSCORE = take(E);
    r.b.BW = reinterpret_cast<int*>(take(E));
    r.total = off;
    return r;
}
extern "C" int64_t echr_beam_ws_floats(const echr_beam_args* ba) {
    if (!ba || ba->beam_size < 1 || ba->seq_len <= 0 || ba->dec.N <= 0 || ba->dec.N % ba->beam_size) return -1;
    echr_dec_args a = ba->dec;
    a.S = ba->seq_len;
    return carve_beam(&a, ba->beam_size, nullptr).total;
}
// bx: the batch extension of echr_decoder_beam_batch (nullptr: one video) -- chain_step's gate products then read the per-row scene part (DecWs)
static int decoder_beam_impl(const echr_beam_args* ba, const echr_batch_ext* bx, void* stream) {
    ECHR_REQUIRE(ba, "decoder_beam: null args");
    RC(persist_check_async());
    DeterministicScope det;                    // `seq` is an index output: bitwise reproducible logits, as the sampler's
    echr_dec_args a = ba->dec;
    const int L = ba->seq_len, B = ba->beam_size;
    ECHR_REQUIRE(L > 0 && ba->seq && ba->seq_logp && ba->score && ba->words && ba->ws_beam && a.ws, "decoder_beam: missing buffers");
    ECHR_REQUIRE(B >= 1 && B <= 16 && B <= a.V1, "decoder_beam: beam_size %d outside [1, min(16, V1)]", B);
    ECHR_REQUIRE(a.N > 0 && a.N % B == 0, "decoder_beam: dec.N = %d is not events * beam_size (%d)", a.N, B);
    ECHR_REQUIRE(!a.rows_disjoint, "decoder_beam: the B rows of an event share its clip rows (rows_disjoint must be 0)");
    a.S = L;                                   // workspace is carved for seq_len steps
    RC(check_dims(&a, "decoder_beam"));
    hipStream_t st = (hipStream_t)stream;
    const int N = a.N, H = a.H, E = N / B;
    DecWs w = carve_ws(&a, a.ws, bx);
    const BeamWs bw = carve_beam(&a, B, ba->ws_beam);
    const DropCfg none = make_drop(nullptr, 0.f);
    {
        float* zp[5] = {w.HS, w.CS[0], w.CS[1], w.CS[2], reinterpret_cast<float*>(bw.s.IT)};          // zero state, <bos> = 0
        long zn[5] = {(long)N * 3 * H, (long)N * H, (long)N * H, (long)N * H, N};
        RC(fill_zero_multi(zp, zn, 5, st));
    }
    if (a.h0) RC(init_state_copy(&a, w, st));
    const bool big = config().gemm_h2 && N >= SAMP_SLAB_ROWS;
    RC(chain_setup(a, w, bw.s, big, st));
    for (int t = 0; t < L; ++t) {
        bool slab_form = false;
        RC(chain_step(a, w, bw.s, t, big, none, none, true, &slab_form, st));
        // the only per-row carries of the chain across steps: h / c after step t (HS[t+1], CS[k][t+1]) and the next tokens (IT)
        const long o = (long)(t + 1) * N;
        RC(beam_step(bw.s.LOGITS, a.V1, E, B, t, L, bw.s.IT, bw.b, w.HS + o * 3 * H, w.CS[0] + o * H, w.CS[1] + o * H, w.CS[2] + o * H, H, st));
    }
    return beam_finalize(bw.b, E, L, reinterpret_cast<long long*>(ba->seq), ba->seq_logp, ba->score, ba->words, st);
}
extern "C" int echr_decoder_beam(const echr_beam_args* ba, void* stream) { return decoder_beam_impl(ba, nullptr, stream); }
// multi-video batch: the same chain called with the extension, then the per-video result widths behind beam_finalize on the same stream
extern "C" int echr_decoder_beam_batch(const echr_beam_args* ba, const echr_batch_ext* x, int32_t* video_words, void* stream) {
    ECHR_REQUIRE(ba && video_words, "decoder_beam_batch: null args / video_words");
    RC(check_batch(&ba->dec, x, "decoder_beam_batch"));
    RC(decoder_beam_impl(ba, x, stream));
    return beam_video_words(ba->words, x->vid, ba->dec.N / ba->beam_size, ba->beam_size, x->n_videos, video_words, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------
// one decoder timestep with the state passed in and out (OldModel.get_logprobs_state, OldModel_NEW.py:133-137): the building block the
// reference's forward()/sample() loop over.  Inference-style entry (no saved activations for a backward pass); bitwise reproducible.
// ------------------------------------------------------------------------------------------------------
static int copy2d(float* dst, long dpitch, const float* src, long spitch, long width, long height, hipStream_t st) {
    if (hipMemcpy2DAsync(dst, dpitch * sizeof(float), src, spitch * sizeof(float), width * sizeof(float), height, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("decoder_step: state copy failed");
        return -5;
    }
    return 0;
}

extern "C" int echr_decoder_step(const echr_dec_args* a0, const float* h_in, const float* c_in, float* h_out, float* c_out,
                                 const echr_dropout* drop, void* stream) {
    RC(persist_check_async());
    ECHR_REQUIRE(a0 && h_in && c_in && h_out && c_out, "decoder_step: null arguments");
    echr_dec_args a = *a0;
    a.S = 1;
    RC(check_dims(&a, "decoder_step"));
    ECHR_REQUIRE(a.ws && a.logp && a.tokens, "decoder_step: missing buffers (ws from echr_decoder_ws_floats with S = 1, logp [N,V1], tokens [N])");
    DeterministicScope det;
    hipStream_t st = (hipStream_t)stream;
    const int N = a.N, H = a.H, E = a.E;
    DecWs w = carve_ws(&a, a.ws);
    const DropCfg dh = make_drop(drop, drop ? drop->p_h : 0.f), dout = make_drop(drop, drop ? drop->p_out : 0.f);
    for (int k = 0; k < 3; ++k) {
        RC(copy2d(w.HS + k * H, 3 * H, h_in + (long)k * N * H, H, H, N, st));          // [3,N,H] -> h(t-1) rows [N,3H]
        RC(copy2d(w.CS[k], H, c_in + (long)k * N * H, H, H, N, st));
    }
    RC(precompute_static(&a, w, st, true));
    RC(embed_gather(a.embed, a.tokens, w.XT, N, E, a.V1, st));
    RC(input_gates(&a, w, w.XT, 0, 1, st));
    RC(step_fwd(&a, w, 0, dh, dout, st));
    echr_gemm_desc d = desc_nt(w.OUTD, 3 * H, a.w_logit, 3 * H, a.logp, a.V1, N, a.V1, 3 * H);
    d.bias = a.b_logit; d.split_k = 1;
    RC(gemm(d, st));
    RC(logsoftmax_rows(a.logp, a.V1, N, 1, 0, 1, a.V1, st));
    for (int k = 0; k < 3; ++k) {
        RC(copy2d(h_out + (long)k * N * H, H, w.HS + (long)N * 3 * H + k * H, 3 * H, H, N, st));
        RC(copy2d(c_out + (long)k * N * H, H, w.CS[k] + (long)N * H, H, H, N, st));
    }
    return 0;
}
