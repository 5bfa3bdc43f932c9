// One training iteration of the caption hot path as ONE library call (echr_train_step, include/echr_hip.h).
//
// Reference protocol: train.py:281-283 (zero_grad), :298 (cg_model forward = CaptionGenerator.py:17-30), :300 (LanguageModelCriterion,
// misc/utils.py:66-75), :313 (backward), :315-317 (clip_gradient + optimizer.step).  The pieces are the library's own entry points
// (event pooling, TSRM encoder, decoder forward, criterion, decoder backward with the fused criterion gradient, TSRM backward,
// clamp + Adam); what this file adds is the sequencing that echr_amd/functional.py + autograd otherwise do from Python -- ~75 ctypes
// calls, four autograd nodes and their callbacks per iteration, 1.2 ms of host time against 1.75 ms of GPU time -- as host C++:
// one call, the index vectors staged through a pinned ring, every buffer carved from one caller-owned workspace.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

static inline long up64(long n) { return (n + 63) / 64 * 64; }
struct StepWs { long idx, ech, tsrm_ws, event, logp, dec_ws, dec_ws_bwd, g_event, g_ech, tsrm_ws_bwd, h0, g_h0, init_feats, init_dfeats, g_video, g_video_init,
                 init_vlen, rows, row_grad, batch, total; };

static inline int init_feats_width(const echr_train_step_args* a) {
    return (a->init_use_v ? a->dec.Dv : 0) + (a->init_use_e ? a->dec.De : 0) + (a->init_use_c ? a->dec.D : 0);
}

// One call of any of the six entries (echr_train_step and _rw, _clip, _batch, _batch_tap, _batch_clip): what the entry was handed, and
// the rules it checks in the order it checks them (validate_step).
// rw: the criterion is weighted -- the index region holds the weights [N,S] too (host_nll = 1), or rw_dev is their device form
// x: 'CH' / 'CC+CH' -- the 'CC+CH' row source [Tv, Dc + Ht] and the clip-row gradient's scratch
// bx: a multi-video batch -- the index region ends with vid [N]; the batch scratch (echr_batch_ws_floats) is carved here too
enum StepRule : char { R_END, R_CLIP, R_BATCH, R_ROWS, R_WIDTH, R_WEIGHTS, R_PREPARED, R_BATCHED, R_HANDOVER, R_INIT_C, R_TAP, R_TAP_BWD, R_VH };
struct StepCall {
    const echr_train_step_args* a; const char* name; const StepRule* rules;          // (name: the entry's suffix, for messages)
    const char* no_prepare = nullptr;          // why a single-video entry refuses prepared = 1 (R_PREPARED on its list)
    bool rw = false; const float* rw_dev = nullptr; const echr_clip_step_args* x = nullptr; const echr_batch_ext* bx = nullptr;
    float* video_loss = nullptr; const int32_t* row_offset = nullptr;
    bool no_g_tap = false;                     // echr_train_step_batch: g_tap is refused (R_TAP on the list: required; otherwise either way)
};

static StepWs carve_step(const StepCall& c) {
    const echr_train_step_args* a = c.a; const echr_clip_step_args* x = c.x; const echr_batch_ext* bx = c.bx; const bool rw = c.rw;
    StepWs w;
    long off = 0;
    auto take = [&](long n) { long o = off; off += up64(n); return o; };
    const echr_tsrm_args& t = a->tsrm;
    const echr_dec_args& d = a->dec;
    w.idx = take((long)(3 + (rw ? 5 : 4) * d.S) * d.N + (bx ? (long)d.N : 0));  // int32: ev_start | ev_len | ind | tokens [S,N] | active rows [<= S*N] | targets [N,S] | mask fp32 [N,S]
                                                          // (| weights fp32 [N,S] with rw)
    // (event_direct: 'EC' / 'EH' -- the pooled / gathered rows ARE the event vectors; no encoder input, workspace or gradients; tsrm is not read)
    const bool direct = a->event_direct != 0;
    w.ech = direct ? -1 : take((long)t.N * t.Din);
    w.tsrm_ws = direct ? -1 : take(echr_tsrm_ws_floats(t.N, t.Din, t.Df, t.Do, t.G));
    w.event = direct ? take((long)d.N * d.De) : take((long)t.N * t.Do);
    w.logp = take((long)d.N * d.S * d.V1);
    w.dec_ws = take(echr_decoder_ws_floats(&d));
    w.dec_ws_bwd = take(echr_decoder_ws_bwd_floats(&d));
    w.g_event = take((long)d.N * d.De);
    w.g_ech = direct ? -1 : take((long)t.N * t.Din);
    w.tsrm_ws_bwd = direct ? -1 : take(echr_tsrm_ws_bwd_floats(t.N, t.Din, t.Df, t.Do, t.G));
    // non-recipe options: initial state (h0, its gradient, init_linear's input rows and their gradient), d video
    w.h0 = w.g_h0 = w.init_feats = w.init_dfeats = -1;
    if (a->w_init) {
        const long h3 = 3L * d.H, dt = init_feats_width(a);
        w.h0 = take((long)d.N * h3); w.g_h0 = take((long)d.N * h3); w.init_feats = take((long)d.N * dt); w.init_dfeats = take((long)d.N * dt);
    }
    // (a batch: d video is [V, Dv]; with an initial state so is init_linear's, and the per-video padded clip lengths [V] int32 are formed here)
    w.g_video = take((bx ? (long)bx->n_videos : 1L) * d.Dv); w.g_video_init = take(((bx && a->w_init) ? (long)bx->n_videos : 1L) * d.Dv);
    w.init_vlen = (bx && a->w_init) ? take(bx->n_videos) : -1;
    w.rows = w.row_grad = -1;
    if (x) {
        if (x->clip_parts == 3) w.rows = take((long)d.Tv * d.D);
        w.row_grad = take(echr_decoder_row_grad_ws_floats(&d, a->Ht > 0 ? a->Ht : 1));
    }
    w.batch = bx ? take(echr_batch_ws_floats(d.N, bx->n_videos, d.H)) : -1;
    w.total = off;
    return w;
}

// Host -> device staging of the per-iteration index vectors: a ring of pinned buffers, each guarded by the event recorded behind the
// copy that reads it, so the host may run several iterations ahead of the GPU without ever rewriting a buffer a copy still reads.
struct PinRing {
    static constexpr int SLOTS = 8;
    void* buf[SLOTS] = {};
    size_t cap[SLOTS] = {};
    hipEvent_t done[SLOTS] = {};
    bool used[SLOTS] = {};
    int next = 0;
};
static PinRing& ring() { static PinRing r; return r; }
static hipEvent_t& ring_last() { static hipEvent_t e = nullptr; return e; }          // the event behind the last staging copy

__global__ __launch_bounds__(256) void stage_copy_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = __builtin_nontemporal_load(src + i);
}
static int stage_indices(const int32_t* host, int32_t* dev, size_t bytes, hipStream_t st) {
    PinRing& r = ring();
    const int s = r.next;
    r.next = (r.next + 1) % PinRing::SLOTS;
    if (r.used[s] && hipEventSynchronize(r.done[s]) != hipSuccess) { set_error("train_step: staging event failed"); return -5; }
    if (r.cap[s] < bytes) {
        if (r.buf[s]) (void)hipHostFree(r.buf[s]);
        r.buf[s] = nullptr; r.cap[s] = 0;
        const size_t want = bytes < 65536 ? 65536 : bytes * 2;
        if (hipHostMalloc(&r.buf[s], want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); set_error("train_step: pinned staging buffer (%zu bytes) unavailable", want); return -12; }
        r.cap[s] = want;
    }
    if (!r.done[s] && hipEventCreateWithFlags(&r.done[s], echr::sync_event_flags()) != hipSuccess) { set_error("train_step: event create failed"); return -5; }
    memcpy(r.buf[s], host, bytes);
    // the pinned buffer is read by a copy KERNEL (host-coherent memory is device-visible at the same address): an in-stream launch of ~3 us.
    // hipMemcpyAsync takes the DMA-engine path for transfers of this size (~19 KB), whose start-up latency (tens of us) sat at the head of
    // every iteration in front of everything else
    const int n = (int)(bytes / 4);
    hipLaunchKernelGGL(stage_copy_kernel, dim3((n + 255) / 256), dim3(256), 0, st, static_cast<const int32_t*>(r.buf[s]), dev, n);
    if (hipGetLastError() != hipSuccess) { set_error("train_step: index upload failed"); return -5; }
    if (hipEventRecord(r.done[s], st) != hipSuccess) { (void)hipGetLastError(); set_error("train_step: index upload failed"); return -5; }
    r.used[s] = true;
    ring_last() = r.done[s];
    return 0;
}

// Stage-ahead (round 6): the LAST kernel of an iteration is clamp + Adam, ~95 us of pure HBM streaming on the caller's stream, and the FIRST
// things of the next one -- the index staging copy and, behind it, the event encoder's position embedding (indices only: the head of the chain
// the forward recurrence waits for) -- need nothing that update writes.  When a call ends with its own update it records an event in front of
// it (every reader of the workspace and the index region is complete there: the helper streams were just joined); the next call on the same
// stream, workspace and arena stages its indices on the TAIL stream behind that event, so that copy and embedding run beside the update, and
// orders everything else behind the caller's stream's position at its entry (the update and whatever the caller queued since).
struct StageAhead { hipEvent_t pre = nullptr, post = nullptr; bool valid = false; hipStream_t st = nullptr; const void* ws = nullptr; const void* flat_g = nullptr; bool init = false, ok = false; };
static StageAhead& stage_ahead() {
    static StageAhead s;
    if (!s.init) {
        s.init = true;
        const char* e = getenv("ECHR_STAGE_AHEAD");          // A/B switch
        s.ok = !(e && e[0] == '0') && hipEventCreateWithFlags(&s.pre, echr::sync_event_flags()) == hipSuccess &&
               hipEventCreateWithFlags(&s.post, echr::sync_event_flags()) == hipSuccess;
        if (!s.ok) (void)hipGetLastError();
    }
    return s;
}

}  // namespace echr

using namespace echr;

#define RC(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

// ---- the six entries: their descriptors and the one validator --------------------------------------------------------------------
//   entry          g_tap      prepared                     defer_update / mid_cb      rules, in the entry's own order: RULES_* below
//   ""             either     taken                        taken
//   "_rw"          either     refused (no weights there)   taken
//   "_clip"        either     refused (rows = tap_feats)   taken
//   "_batch"       REFUSED    refused                      defer refused, mid unread
//   "_batch_tap"   REQUIRED   refused                      both refused
//   "_batch_clip"  either     refused                      both refused
static const StepRule RULES_PLAIN[] = {R_END}, RULES_RW[] = {R_WEIGHTS, R_PREPARED, R_END},
                      RULES_CLIP[] = {R_CLIP, R_ROWS, R_WIDTH, R_PREPARED, R_INIT_C, R_WEIGHTS, R_END},
                      RULES_BATCH[] = {R_BATCH, R_WEIGHTS, R_BATCHED, R_HANDOVER, R_END},
                      RULES_BATCH_TAP[] = {R_BATCH, R_WEIGHTS, R_TAP, R_VH, R_BATCHED, R_HANDOVER, R_END},
                      RULES_BATCH_CLIP[] = {R_CLIP, R_BATCH, R_ROWS, R_WIDTH, R_WEIGHTS, R_BATCHED, R_HANDOVER, R_INIT_C, R_TAP_BWD, R_VH, R_END};

static StepCall plain_call(const echr_train_step_args* a) { return StepCall{a, "", RULES_PLAIN}; }
static StepCall rw_call(const echr_train_step_args* a, const float* weight = nullptr) {
    return StepCall{a, "_rw", RULES_RW, "echr_train_step_prepare does not take the weights", true, weight};
}
static StepCall clip_call(const echr_train_step_args* a, const echr_clip_step_args* x) {
    const bool rw = x && x->rw;
    return StepCall{a, "_clip", RULES_CLIP, "the clip rows are tap_feats: echr_train_step_prepare cannot run ahead of them", rw, rw ? x->weight : nullptr, x};
}
static StepCall batch_call(const echr_train_step_args* a, const echr_batch_ext* bx, const float* weight = nullptr, float* video_loss = nullptr) {
    StepCall c{a, "_batch", RULES_BATCH};
    c.rw = c.no_g_tap = true; c.rw_dev = weight; c.bx = bx; c.video_loss = video_loss;
    return c;
}
static StepCall batch_tap_call(const echr_train_step_args* a, const echr_batch_ext* bx, const float* weight, float* video_loss, const int32_t* row_offset) {
    StepCall c = batch_call(a, bx, weight, video_loss); c.name = "_batch_tap"; c.rules = RULES_BATCH_TAP; c.no_g_tap = false; c.row_offset = row_offset;
    return c;
}
static StepCall batch_clip_call(const echr_train_step_args* a, const echr_clip_step_args* x, const echr_batch_ext* bx, const float* weight = nullptr,
                                float* video_loss = nullptr, const int32_t* row_offset = nullptr) {
    StepCall c = batch_tap_call(a, bx, weight, video_loss, row_offset); c.name = "_batch_clip"; c.rules = RULES_BATCH_CLIP; c.x = x;
    return c;
}
static int check_n_active(const echr_train_step_args* a) {
    ECHR_REQUIRE(a->n_active >= 0 && a->n_active <= a->dec.S * a->dec.N, "train_step: n_active out of range");
    return 0;
}

// every argument rule of the entries, each stated once; an entry checks the ones on its list, in that order
static int validate_step(const StepCall& c) {
    const echr_train_step_args* a = c.a; const echr_clip_step_args* x = c.x; const echr_batch_ext* bx = c.bx; const char* n = c.name;
    for (const StepRule* r = c.rules; *r != R_END; ++r) switch (*r) {
    case R_CLIP: ECHR_REQUIRE(a && x && (x->clip_parts == 2 || x->clip_parts == 3), "train_step%s: clip_parts must be 2 ('CH') or 3 ('CC+CH')", n); break;
    case R_BATCH: ECHR_REQUIRE(a && bx && bx->n_videos > 0 && bx->n_videos <= a->dec.N && bx->video, "train_step%s: the batch extension needs 0 < n_videos <= N and video", n); break;
    case R_ROWS: ECHR_REQUIRE(x->c3d && x->Dc > 0 && a->tap && a->Ht > 0, "train_step%s: c3d / tap missing", n); break;
    case R_WIDTH: ECHR_REQUIRE(a->dec.D == (x->clip_parts == 3 ? x->Dc + a->Ht : a->Ht), "train_step%s: dec.D = %d is not the width of the clip rows", n, a->dec.D); break;
    case R_WEIGHTS:          // (after this rule rw_dev is the device weight or, with host_nll = 1, NULL)
        if (!c.rw) break;
        ECHR_REQUIRE(a && (a->host_nll || c.rw_dev), "train_step%s: the criterion weights are missing (device `weight`, or host_index with host_nll = 1)", n);
        ECHR_REQUIRE(!(a->host_nll && c.rw_dev), "train_step%s: host_nll = 1 carries the weights in host_index: pass weight = NULL", n);
        break;
    case R_PREPARED: ECHR_REQUIRE(!a->prepared, "train_step%s: %s (prepared must be 0)", n, c.no_prepare); break;
    case R_BATCHED:          // (echr_train_step_batch never reads mid_cb: the form that calls it needs g_tap)
        ECHR_REQUIRE(!a->prepared && !a->defer_update && !(c.no_g_tap ? (const void*)a->g_tap : (const void*)a->mid_cb),
                     "train_step%s: prepared, defer_update and %s are not part of the batched step", n, c.no_g_tap ? "g_tap" : "mid_cb");
        break;
    case R_HANDOVER: ECHR_REQUIRE(!a->handover || !a->do_step, "train_step%s: handover = 1 needs do_step = 0 (the caller reduces the gradients, then steps)", n); break;
    case R_INIT_C: ECHR_REQUIRE(!(a->w_init && a->init_use_c), "train_step%s: an initial state that reads the clip has no row gradient", n); break;
    case R_TAP: ECHR_REQUIRE(a->g_tap && a->tap && a->Ht > 0 && !a->forward_only, "train_step%s: g_tap / tap missing (without g_tap this is echr_train_step_batch)", n); break;
    case R_TAP_BWD: ECHR_REQUIRE(!a->g_tap || !a->forward_only, "train_step%s: g_tap needs the backward pass (forward_only must be 0)", n); break;
    case R_VH: ECHR_REQUIRE(!a->g_tap || a->vh_offset < 0 || c.row_offset, "train_step%s: the 'VH' scene gradient needs row_offset", n); break;
    case R_END: break;
    }
    return 0;
}

// diagnostic (ECHR_STEP_TIMING=1): HIP events at the phase boundaries of the call on the caller's stream; every 50th call prints the averages
struct StepTiming { hipEvent_t e[6][8] = {}; int calls = 0; bool on = false, init = false; double acc[5] = {0, 0, 0, 0, 0}; int n = 0; };
static StepTiming& step_timing() {
    static StepTiming t;
    if (!t.init) {
        t.init = true;
        const char* e = getenv("ECHR_STEP_TIMING");
        t.on = e && e[0] == '1';
        if (t.on) for (auto& row : t.e) for (auto& ev : row) if (hipEventCreate(&ev) != hipSuccess) t.on = false;
    }
    return t;
}
static void step_mark(int k, hipStream_t st) {
    StepTiming& t = step_timing();
    if (t.on) (void)hipEventRecord(t.e[k][t.calls % 8], st);
}
static void step_timing_end() {
    StepTiming& t = step_timing();
    if (!t.on) return;
    const int slot = (t.calls + 1) % 8;          // the oldest recorded call: long finished
    if (t.calls >= 8) {
        float ms;
        bool ok = true;
        double d[5];
        for (int k = 0; k < 5 && ok; ++k) { ok = hipEventElapsedTime(&ms, t.e[k][slot], t.e[k + 1][slot]) == hipSuccess; d[k] = ms; }
        if (ok) { for (int k = 0; k < 5; ++k) t.acc[k] += d[k]; ++t.n; } else (void)hipGetLastError();
    }
    ++t.calls;
    if (t.n && t.calls % 50 == 0) {
        fprintf(stderr, "[train_step] encoder + forward (to d logits) %.3f ms | decoder backward on this stream %.3f | event encoder backward %.3f | wait for the helper streams %.3f | clamp + Adam %.3f\n",
                t.acc[0] / t.n, t.acc[1] / t.n, t.acc[2] / t.n, t.acc[3] / t.n, t.acc[4] / t.n);
        for (double& x : t.acc) x = 0;
        t.n = 0;
    }
}

// joint mode: the helper streams' work of one call
struct JointPending { echr_dec_args d; echr_dec_grads g; echr_tsrm_args t; echr_tsrm_grads tg; echr_dropout drop; echr_train_step_args args;
                      DecCall call; };          // (call: the decoder call of the first piece -- echr_train_step_rw's criterion weight; one video, no hand-over)
// every parameter gradient (decoder: helper streams forked from `src`; event encoder: behind them on the prepare stream), then clamp + Adam on
// the tail stream, published for echr_stream_join
static int joint_finish(JointPending& jp, hipStream_t src) {
    RC(decoder_bwd_parts(&jp.d, &jp.g, &jp.drop, src, 2, jp.call));
    hipStream_t s2 = aux2_stream();
    RC(tsrm_bwd_parts(&jp.t, &jp.tg, &jp.drop, s2, 2));
    hipStream_t ts = helpers_merge_to_tail();
    if (!ts) return -5;
    const echr_train_step_args& a = jp.args;
    RC(echr_clamp_adam_counted(a.flat_p, a.flat_g, a.adam_m, a.adam_v, a.n_flat, a.adam_step, a.lr, a.beta1, a.beta2, a.eps, a.clip, a.adam_applied, ts));
    return tail_publish();
}

// the decoder arguments of one call (shared by echr_train_step_prepare and echr_train_step: both must describe the same launch)
static echr_dec_args step_dec_args(const echr_train_step_args* a, const StepWs& L, const int32_t* idx) {
    const int N = a->dec.N;
    echr_dec_args d = a->dec;
    d.ev_start = idx; d.ev_len = idx + N; d.tokens = idx + 3 * N;
    d.ws = a->ws + L.dec_ws; d.logp = a->ws + L.logp; d.event = nullptr; d.prepared = 0;
    d.train = a->forward_only ? 0 : 1;
    // the gradient arena is zero-filled by the forward's first fill launch (beside the event encoder), not in front of the reverse recurrence
    d.zero_extra = a->forward_only ? nullptr : a->flat_g; d.zero_extra_count = a->n_flat;
    // (the initial-state buffer is filled behind the event encoder; its ADDRESS is part of the description from the start, so that the prepare
    // half and the forward agree on which recurrence kernels run -- the persistent ones start from zero and decline h0)
    d.h0 = a->w_init ? a->ws + L.h0 : nullptr;
    return d;
}
// the staged index region in int32 words: what every call stages (the offset of a batch's vid), and with vid [N] behind it
static size_t step_vid_offset(const StepCall& c) {
    const echr_train_step_args* a = c.a;
    return (size_t)(3 + a->dec.S) * a->dec.N + (size_t)a->n_active + (a->host_nll ? (c.rw ? 3 : 2) * (size_t)a->dec.S * a->dec.N : 0);
}
static size_t step_index_count(const StepCall& c) { return step_vid_offset(c) + (c.bx ? (size_t)c.a->dec.N : 0); }

// Optional first half of echr_train_step for the joint 'tap_cg' iteration (train.py:300-313): everything of the call that does not read
// tap_feats -- index staging and the decoder's event-independent part (attention projections of the video, token-side gates, operand packs,
// the gradient-arena fill) -- is started on the library's prepare stream BEFORE the caller queues the proposal encoder's forward, a 64-workgroup
// persistent launch that leaves three quarters of the chip idle.  The following echr_train_step takes the same arguments plus prepared = 1
// (tap / g_tap may be filled in only then).
extern "C" int echr_train_step_prepare(const echr_train_step_args* a, void* stream) {
    ECHR_REQUIRE(a && a->ws && a->host_index && a->flat_g, "train_step_prepare: missing buffers");
    ECHR_REQUIRE(a->overlap_encoder, "train_step_prepare: needs overlap_encoder = 1");
    ECHR_REQUIRE(!a->event_direct, "train_step_prepare: event_direct = %d ('EC' / 'EH') runs without the prepare half (call echr_train_step with prepared = 0)", a->event_direct);
    hipStream_t st = (hipStream_t)stream;
    RC(join_tail(st));
    const StepCall c = plain_call(a);
    const StepWs L = carve_step(c);
    ECHR_REQUIRE(a->ws_floats >= L.total, "train_step_prepare: workspace holds %lld floats, %ld needed (echr_train_step_ws_floats)", (long long)a->ws_floats, L.total);
    RC(check_n_active(a));
    int32_t* idx = reinterpret_cast<int32_t*>(a->ws + L.idx);
    RC(stage_indices(a->host_index, idx, sizeof(int32_t) * step_index_count(c), st));
    echr_dec_args d = step_dec_args(a, L, idx);
    // the event encoder's position branch reads indices and parameters only: it starts here too, not with the second half behind the proposal
    // encoder's forward, where its ~70 us chain would sit in front of the forward recurrence
    echr_tsrm_args t = a->tsrm;
    t.ech = a->ws + L.ech; t.ev_start = idx; t.ev_len = idx + a->dec.N; t.ws = a->ws + L.tsrm_ws; t.out = a->ws + L.event;
    t.inference = 0; t.max_len = 0; t.max_span = 0;
    int rc = tsrm_position_early(&t, st);
    if (!rc) rc = echr_decoder_fwd_prepare(&d, stream);
    if (rc) { (void)tsrm_position_early(nullptr, nullptr); (void)aux_join(st); }
    return rc;
}

static int train_step_impl(const StepCall& c, void* stream);          // validate_step, then the iteration
extern "C" int64_t echr_train_step_ws_floats(const echr_train_step_args* a) { return a ? carve_step(plain_call(a)).total : -1; }
extern "C" int echr_train_step(const echr_train_step_args* a, void* stream) { return train_step_impl(plain_call(a), stream); }
// Frame-level context 'CH' / 'CC+CH' (include/echr_hip.h): the same iteration with tap_feats (or [c3d | tap]) as the attended rows and the
// clip-row gradient added to g_tap behind the join of the backward's helper streams
extern "C" int64_t echr_train_step_clip_ws_floats(const echr_train_step_args* a, const echr_clip_step_args* x) {
    return (a && x) ? carve_step(clip_call(a, x)).total : -1;
}
extern "C" int echr_train_step_clip(const echr_train_step_args* a, const echr_clip_step_args* x, void* stream) { return train_step_impl(clip_call(a, x), stream); }
// Self-critical training (RewardCriterion, misc/utils.py:48-59): the same iteration with the criterion's numerator weighted by the signed
// rw[n,t] = reward * mask.  Stage-ahead needs no extra guard here: the decodes a caller runs between two calls (the sampled and the greedy pass,
// the event context they read) use workspaces of their own and never this call's `ws`, index ring or gradient arena, and they are queued on
// the caller's stream behind the update they read the parameters of; the next call's staging is the only work that runs beside that update,
// and everything else of it is ordered behind the caller's stream's position at its entry, i.e. behind those decodes.
extern "C" int64_t echr_train_step_rw_ws_floats(const echr_train_step_args* a) { return a ? carve_step(rw_call(a)).total : -1; }
extern "C" int echr_train_step_rw(const echr_train_step_args* a, const float* weight, void* stream) { return train_step_impl(rw_call(a, weight), stream); }
// Multi-video batch (include/echr_hip.h): the same iteration over the events of V videos.  What differs sits in the pieces the call sequences --
// per-video scene vectors and their segmented gradients (decoder.hip), the block-diagonal event encoder (tsrm.hip), the criterion's
// per-video normalisers inside the weights (core.hip) -- which are handed the extension as an argument (DecCall.bx, vid, unit_den); this file
// stages vid with the other index vectors and adds the per-video losses.  Stage-ahead, the applied-update count and the asynchronous failure reports are
// those of echr_train_step: the same code runs.
extern "C" int64_t echr_train_step_batch_ws_floats(const echr_train_step_args* a, const echr_batch_ext* x) {
    return (a && x && x->n_videos > 0) ? carve_step(batch_call(a, x)).total : -1;
}
extern "C" int echr_train_step_batch(const echr_train_step_args* a, const echr_batch_ext* x, const float* weight, float* video_loss, void* stream) {
    return train_step_impl(batch_call(a, x, weight, video_loss), stream);
}
// The joint 'tap_cg' iteration over a batch: echr_train_step_batch that also returns d loss / d tap_feats.  a->g_tap [T_tot, Ht] is zero-filled
// by the caller and added into: the anchors' rows through the block-diagonal event encoder's d ech (ind is batch-absolute; 'ER1' reads no
// tap row and adds nothing), and with 'VH' each video's d scene vector spread over that video's OWN rows (row_offset, device [V+1]).
extern "C" int64_t echr_train_step_batch_tap_ws_floats(const echr_train_step_args* a, const echr_batch_ext* x) {
    return echr_train_step_batch_ws_floats(a, x);
}
extern "C" int echr_train_step_batch_tap(const echr_train_step_args* a, const echr_batch_ext* x, const float* weight, float* video_loss,
                                         const int32_t* row_offset, void* stream) {
    return train_step_impl(batch_tap_call(a, x, weight, video_loss, row_offset), stream);
}
// The frame-level contexts over a batch: echr_train_step_batch (and, with g_tap, echr_train_step_batch_tap) with the row source of
// echr_train_step_clip over the T_tot concatenated rows.  ev_start is batch-absolute, so the attention, its backward and the clip-row gradient
// address the rows as they do for one video; g_tap gains the anchors' rows, the 'VH' span over each video's own rows and the clip-row gradient.
extern "C" int64_t echr_train_step_batch_clip_ws_floats(const echr_train_step_args* a, const echr_clip_step_args* x, const echr_batch_ext* bx) {
    const bool ok = a && x && bx && bx->n_videos > 0 && (x->clip_parts == 2 || x->clip_parts == 3);
    return ok ? carve_step(batch_clip_call(a, x, bx)).total : -1;
}
extern "C" int echr_train_step_batch_clip(const echr_train_step_args* a, const echr_clip_step_args* x, const echr_batch_ext* bx, const float* weight,
                                          float* video_loss, const int32_t* row_offset, void* stream) {
    return train_step_impl(batch_clip_call(a, x, bx, weight, video_loss, row_offset), stream);
}
static int train_step_impl(const StepCall& c, void* stream) {
    RC(validate_step(c));
    const echr_train_step_args* a = c.a; const echr_clip_step_args* x = c.x; const echr_batch_ext* bx = c.bx; const bool rw = c.rw;
    float* video_loss = c.video_loss; const int32_t* row_offset = c.row_offset;
    // event_direct ('EC' / 'EH', include/echr_hip.h): the event vectors without the event encoder; its own rules first, each with its own message
    const int direct = a ? a->event_direct : 0;
    if (direct) {
        ECHR_REQUIRE(direct >= 1 && direct <= 2, "train_step: event_direct = %d: 0 (through the event encoder), 1 ('EC') or 2 ('EH')", direct);
        ECHR_REQUIRE(direct != 2 || (a->tap && a->Ht > 0), "train_step: event_direct = 2 ('EH') reads the anchors' rows of tap: tap / Ht missing");
        const int want = direct == 1 ? (x ? x->Dc : a->dec.D) : a->Ht;
        ECHR_REQUIRE(a->dec.De == want, "train_step: event_direct = %d: dec.De = %d is not the width of the %s (%d)", direct, a->dec.De,
                     direct == 1 ? "C3D rows" : "proposal encoder's states", want);
        ECHR_REQUIRE(!a->prepared, "train_step: event_direct = %d runs without echr_train_step_prepare (prepared must be 0)", direct);
    }
    ECHR_REQUIRE(a && a->ws && a->host_index && a->loss && a->g_loss && a->flat_g && (a->tap || a->event_parts == 1 || direct == 1), "train_step: missing buffers");
    ECHR_REQUIRE(!a->prepared || a->overlap_encoder, "train_step: prepared = 1 needs overlap_encoder = 1");
    const int parts = direct ? direct : a->event_parts ? a->event_parts : 3;
    ECHR_REQUIRE(parts >= 1 && parts <= 3, "train_step: event_parts must be 0..3");
    const int Dc = x ? x->Dc : a->dec.D;          // (the C3D features' width: the row source's one with 'CC')
    const float* c3d = x ? x->c3d : a->dec.c3d;
    const int De_c3d = (parts & 1) ? Dc : 0, De_tap = (parts & 2) ? a->Ht : 0;          // the two halves of the event encoder's input rows
    ECHR_REQUIRE(direct || (a->tsrm.N == a->dec.N && a->tsrm.Do == a->dec.De && a->tsrm.Din == De_c3d + De_tap), "train_step: encoder / decoder shapes disagree");
    const bool vh = a->g_tap && a->vh_offset >= 0;
    ECHR_REQUIRE(!vh || (a->vh_offset + a->Ht <= a->dec.Dv && a->tap_rows > 0), "train_step: vh_offset / tap_rows do not describe a span of dec.video");
    ECHR_REQUIRE(!a->w_init || (a->b_init && (a->forward_only || (a->g_w_init && a->g_b_init)) && init_feats_width(a) > 0), "train_step: init_linear pointers incomplete");
    ECHR_REQUIRE(!a->do_step || (a->flat_p && a->adam_m && a->adam_v && a->adam_step >= 1), "train_step: optimiser state missing");
    hipStream_t st = (hipStream_t)stream;
    RC(join_tail(st));          // (a deferred update of the previous call: it reads the index region this call is about to restage)
    const StepWs L = carve_step(c);
    ECHR_REQUIRE(a->ws_floats >= L.total, "train_step: workspace holds %lld floats, %ld needed (echr_train_step%s_ws_floats)", (long long)a->ws_floats, L.total,
                 c.bx && !c.x ? "_batch" : c.name);
    float* ws = a->ws;
    // 'CC+CH': the row source [c3d | tap] is formed first, ahead of every fork of this call (the decoder's event-independent part reads it)
    if (x && x->clip_parts == 3) RC(clip_rows(c3d, Dc, a->tap, a->Ht, ws + L.rows, a->dec.Tv, st));
    const int N = a->dec.N, S = a->dec.S;
    step_mark(0, st);
    int32_t* idx = reinterpret_cast<int32_t*>(ws + L.idx);
    RC(check_n_active(a));
    StageAhead& sa = stage_ahead();
    const bool ahead = sa.ok && sa.valid && !a->prepared && a->overlap_encoder && sa.st == st && sa.ws == a->ws && sa.flat_g == a->flat_g &&
                       helpers_available() && tail_stream_raw();
    sa.valid = false;          // (consumed, or void: whatever this call does, the recorded pair no longer brackets the stream's last work)
    if (ahead) {
        hipStream_t ts = tail_stream_raw();
        if (hipStreamWaitEvent(ts, sa.pre, 0) != hipSuccess) { set_error("train_step: stream wait failed"); return -5; }
        RC(stage_indices(a->host_index, idx, sizeof(int32_t) * step_index_count(c), ts));
        // the caller's stream: behind the staging copy (its own position is already behind the update).  The prepare stream: behind the
        // caller's stream's position AT ENTRY -- the update, and whatever the caller queued since (this call's inputs: an upload of the next
        // video's features, the proposal encoder's forward; a write to the parameters) -- since the staging event it forks from no longer
        // implies that position
        if (hipEventRecord(sa.post, st) != hipSuccess) { set_error("train_step: event record failed"); return -5; }
        RC(prep_stream_wait(sa.post));
        if (hipStreamWaitEvent(st, ring_last(), 0) != hipSuccess) { set_error("train_step: stream wait failed"); return -5; }
    } else if (!a->prepared) RC(stage_indices(a->host_index, idx, sizeof(int32_t) * step_index_count(c), st));
    // multi-video batch: vid is the tail of the staged index region, the batch scratch a piece of `ws`; everything below that needs the
    // extension is called with it (dc.bx, bxl.vid, unit_den)
    echr_batch_ext bxl;
    if (bx) {
        bxl = *bx;
        bxl.vid = idx + step_vid_offset(c);
        bxl.ws = ws + L.batch;
        if (vh) bxl.g_video = ws + L.g_video;          // [V, Dv]: the batched decoder backward writes d video per video (its spans go into g_tap)
    }
    const int32_t *ev_start = idx, *ev_len = idx + N, *ind = idx + 2 * N, *active = idx + (3 + S) * N;          // (tokens at idx + 3 N: step_dec_args)
    const void* nll_target = a->nll_target;
    const float* nll_mask = a->nll_mask;
    int nll_i64 = a->nll_target_i64;
    const float* crit_w = c.rw_dev;
    if (a->host_nll) {          // targets / mask (/ weights) came with the index vectors
        nll_target = active + a->n_active;
        nll_mask = reinterpret_cast<const float*>(active + a->n_active + (size_t)S * N);
        nll_i64 = 0;
        if (rw) crit_w = reinterpret_cast<const float*>(active + a->n_active + 2 * (size_t)S * N);
    }
    ECHR_REQUIRE(nll_target && nll_mask, "train_step: criterion targets / mask missing");
    DecCall dc;          // the decoder call of this iteration; the backward adds the hand-over request
    dc.bx = bx ? &bxl : nullptr; dc.rw = crit_w;
    const bool unit_den = bx != nullptr;          // a batch: the per-video normalisers arrive inside the criterion weights

    echr_dec_args d = step_dec_args(a, L, idx);
    if (x) d.c3d = x->clip_parts == 3 ? ws + L.rows : a->tap;
    echr_tsrm_args t = a->tsrm;          // (event_direct: described, never launched)
    t.ech = direct ? nullptr : ws + L.ech; t.ev_start = ev_start; t.ev_len = ev_len; t.ws = direct ? nullptr : ws + L.tsrm_ws; t.out = ws + L.event;
    t.inference = 0; t.max_len = 0; t.max_span = 0;
    // the event encoder's position branch (pair embedding -> fc1 -> fc2 gates: indices and parameters only) starts right behind the staging
    // CaptionGenerator.forward (:23-30): the decoder's event-independent part starts on the library's second stream and overlaps the event encoder
    if (a->overlap_encoder && !a->prepared) {
        fork_event(ring_last());          // both forks hang off the staging copy's event: no further record in front of event pooling
        int rc2 = direct ? 0 : tsrm_position_early(&t, st);          // (no encoder, no position branch)
        if (!rc2) rc2 = decoder_fwd_prepare(&d, dc, stream);
        fork_event(nullptr);
        if (rc2) {
            // the position branch may already be queued on the tail stream: forget it (a later echr_tsrm_fwd on this workspace must not take the
            // `early` form with stale gates) and order this stream behind what was queued, as the event encoder's own failure path does
            (void)tsrm_position_early(nullptr, nullptr);
            (void)aux_join(st);
            (void)aux2_join(st);          // (a prepare chain that failed half-way published nothing: join the stream itself)
            (void)echr_decoder_fwd_prepare_cancel(stream);
            return rc2;
        }
    }
    // (event_direct: the pooled rows / the anchors' states are the event vectors themselves, :131-137)
    int rc = echr_event_pool_gather_fwd(c3d, a->tap, ev_start, ev_len, ind, ws + (direct ? L.event : L.ech), N, De_c3d, De_tap, stream);       // :106-128
    if (!rc && !direct) rc = tsrm_fwd_checked(&t, &a->drop, stream, bx ? bxl.vid : nullptr);          // :129
    if (rc) { (void)tsrm_position_early(nullptr, nullptr); if (a->overlap_encoder) (void)echr_decoder_fwd_prepare_cancel(stream); return rc; }
    d.event = ws + L.event; d.prepared = a->overlap_encoder ? 1 : 0;
    // OldModel.init_hidden with CG_init_feats_type (OldModel_NEW.py:72-96): h(-1) = c(-1) = init_linear(cat(selected contexts))
    echr_init_state_args ia;
    memset(&ia, 0, sizeof(ia));
    if (a->w_init) {
        ia.N = N; ia.Dv = a->dec.Dv; ia.De = a->dec.De; ia.D = a->dec.D; ia.H3 = 3 * a->dec.H;
        ia.use_v = a->init_use_v; ia.use_e = a->init_use_e; ia.use_c = a->init_use_c; ia.A = a->dec.A;
        ia.video = a->dec.video; ia.event = ws + L.event; ia.c3d = d.c3d; ia.ev_start = ev_start; ia.ev_len = ev_len;
        ia.w = a->w_init; ia.b = a->b_init; ia.feats = ws + L.init_feats; ia.h0 = ws + L.h0;
        // (a batch: the scene vector of the event's own video and that video's padded clip length, formed on the device from ev_len / vid)
        rc = bx ? echr_init_state_fwd_batch(&ia, &bxl, reinterpret_cast<int32_t*>(ws + L.init_vlen), stream) : echr_init_state_fwd(&ia, stream);
        if (rc) { if (a->overlap_encoder) (void)echr_decoder_fwd_prepare_cancel(stream); return rc; }
    }
    echr_dec_grads g = a->dec_g;
    g.g_event = ws + L.g_event; g.g_logp = nullptr;
    g.nll_target = static_cast<const int32_t*>(nll_target); g.nll_target_i64 = nll_i64; g.nll_mask = nll_mask;
    g.active_rows = a->n_active > 0 ? active : nullptr; g.n_active = a->n_active;
    g.g_loss = a->g_loss; g.nll_msum = a->loss + 1;
    g.g_h0 = a->w_init ? ws + L.g_h0 : nullptr;
    if (vh) g.g_video = ws + L.g_video;          // (the caller's own g_video, if any, is not filled then: the span is routed into g_tap)
    g.ws_bwd = ws + L.dec_ws_bwd; g.zeroed = 1; g.phase = 0; g.async_tail = 2;          // only d event on the caller's stream
    if (!a->forward_only && a->overlap_encoder) RC(decoder_bwd_scratch_ahead(&d, &g));          // the backward's scratch fill: behind the prepare chain, not between the recurrences
    // forward (:30) + LanguageModelCriterion (misc/utils.py:66-75).  Training: log-softmax, criterion and its gradient are ONE pass over the
    // logits (d logits land in the backward workspace, the log-probs are never written; the loss is summed behind the backward pass, where
    // this stream waits for the helper stream anyway).  forward_only: the plain log-softmax + criterion, loss[0] = loss, loss[1] = sum(mask)
    bool fused_nll = false, compact = false;
    if (a->forward_only) RC(decoder_fwd_fused(&d, nullptr, &a->drop, stream, nullptr, nullptr, dc));
    else RC(decoder_fwd_fused(&d, &g, &a->drop, stream, &fused_nll, &compact, dc));          // (dc.rw nullptr: LanguageModelCriterion)
    if (!fused_nll && crit_w) RC(nll_loss_rw(d.logp, nll_target, nll_i64, nll_mask, crit_w, a->loss, N, S, d.V1, st, unit_den));
    else if (!fused_nll) {
        if (nll_i64) RC(echr_nll_loss_fwd_i64(d.logp, static_cast<const int64_t*>(nll_target), nll_mask, a->loss, N, S, d.V1, stream));
        else RC(echr_nll_loss_fwd(d.logp, static_cast<const int32_t*>(nll_target), nll_mask, a->loss, N, S, d.V1, stream));
    }
    // (a statement of its own behind the criterion chain above: the per-video losses of a batch from the log-probs)
    if (bx && video_loss && !fused_nll) RC(video_loss_logp(d.logp, nll_target, nll_i64, crit_w, N, S, d.V1, bxl.vid, bxl.n_videos, video_loss, st));
    if (a->forward_only) return 0;
    step_mark(1, st);
    g.dlg_ready = fused_nll ? 1 : 0;
    if (fused_nll) g.nll_msum = nullptr;
    if (!compact) { g.active_rows = nullptr; g.n_active = 0; }          // (the forward kept all rows: vocabulary beyond the register-resident kernels, h2 off)

    // backward (train.py:313): criterion gradient in fused form
    g.zero_extra = nullptr; g.zero_extra_count = 0;
    handover_clear();          // (hand-over points of an earlier call are void from here on)
    if (a->defer_update && a->g_tap && a->do_step && g.async_tail == 2 && fused_nll && config().gemm_h2 && helpers_available() && !vh && !a->w_init && !x && !direct) {
        // Joint 'tap_cg' iteration (train.py:300-313): the proposal encoder's backward -- a 64-workgroup persistent launch that leaves three
        // quarters of the chip idle -- waits for d tap_feats alone.  The chain that leads to it (late fusion, reverse recurrence, d event,
        // the event encoder's attention backward, d ech) runs first and alone on the caller's stream; every parameter gradient and the
        // clamp + Adam update follow on the helper streams, forked behind it, and are NOT joined here: they overlap whatever the caller
        // queues next.  echr_stream_join (and the next echr_train_step / decoder call) waits for them.
        ECHR_REQUIRE(!bx, "train_step: the deferred update is not part of the batched step");          // (R_BATCHED refuses defer_update: one video from here on)
        echr_tsrm_grads tg = a->tsrm_g;
        tg.g_ech = ws + L.g_ech; tg.g_out = ws + L.g_event; tg.ws_bwd = ws + L.tsrm_ws_bwd; tg.zeroed = 1;
        RC(decoder_bwd_parts(&d, &g, &a->drop, stream, 1, dc));
        RC(tsrm_bwd_parts(&t, &tg, &a->drop, stream, 1));
        if (De_tap > 0) RC(echr_event_pool_gather_bwd(ws + L.g_ech, ind, a->g_tap, N, De_c3d, De_tap, stream));
        RC(decoder_fused_loss(&d, &g, a->loss, st, crit_w != nullptr, unit_den));
        // the caller's hook: the proposal encoder's backward (+ update) goes onto `stream` HERE, right behind g_tap; the helper streams fork
        // behind it (joint_finish), so the chip-filling tail never shares CUs with that 64-workgroup latency chain
        if (a->mid_cb) a->mid_cb(stream, a->mid_user);
        JointPending jp;
        jp.d = d; jp.g = g; jp.t = t; jp.tg = tg; jp.drop = a->drop; jp.args = *a; jp.call = dc;
        // (issuing the helper work only after the caller has queued the proposal encoder's backward -- a second entry point, tried -- is worse:
        // 3.21 vs 3.00 ms on c5.  The host needs ~0.5 ms to get from here to that launch anyway, the helpers fill exactly that gap, and a
        // persistent recurrence that shares its CUs with GEMM workgroups from its first step on loses more than the gap is worth)
        return joint_finish(jp, st);
    }
    // (the hand-over request is part of THIS backward pass: its events stay valid for echr_handover_wait, later backward passes record none)
    dc.handover = a->handover && !a->do_step; dc.handover_cb = a->handover_cb; dc.handover_user = a->handover_user;
    RC(decoder_bwd_checked(&d, &g, &a->drop, stream, dc));
    step_mark(2, st);
    if (a->w_init) {
        // d h0 -> init_linear's gradients, d event (ADDED to what the decoder left there, ahead of the event encoder's backward), d video
        echr_init_state_grads ig;
        ig.g_h0 = ws + L.g_h0; ig.g_w = a->g_w_init; ig.g_b = a->g_b_init; ig.zeroed = 1;
        ig.g_video = (vh && a->init_use_v) ? ws + L.g_video_init : nullptr;
        ig.g_event = a->init_use_e ? ws + L.g_event : nullptr;
        ig.dfeats = ws + L.init_dfeats;
        if (bx) {          // d video per video [V, Dv], a fixed-order segmented sum (wanted for the 'VH' span only, like the decoder's)
            echr_batch_ext bi = bxl;
            bi.g_video = (vh && a->init_use_v) ? ws + L.g_video_init : nullptr;
            RC(echr_init_state_bwd_batch(&ia, &ig, &bi, stream));
        } else
        RC(echr_init_state_bwd(&ia, &ig, stream));
    }
    if (direct) {
        // d event IS the gradient of the pooled / gathered rows: 'EH' scatters it onto the anchors' rows of g_tap, 'EC' reaches data only
        if (a->g_tap && De_tap > 0) RC(echr_event_pool_gather_bwd(ws + L.g_event, ind, a->g_tap, N, 0, De_tap, stream));
    } else {
        echr_tsrm_grads tg = a->tsrm_g;
        // d ech (the gradient of the event encoder's INPUT rows) only matters when d tap_feats is asked for: c3d features are data
        tg.g_ech = (a->g_tap && De_tap > 0) ? ws + L.g_ech : nullptr; tg.g_out = ws + L.g_event; tg.ws_bwd = ws + L.tsrm_ws_bwd; tg.zeroed = 1;
        RC(echr_tsrm_bwd(&t, &tg, &a->drop, stream));
        if (a->g_tap && De_tap > 0) RC(echr_event_pool_gather_bwd(ws + L.g_ech, ind, a->g_tap, N, De_c3d, De_tap, stream));
    }
    if (fused_nll) RC(decoder_fused_loss(&d, &g, a->loss, st, crit_w != nullptr, unit_den));
    if (fused_nll && bx && video_loss) RC(decoder_fused_video_loss(&d, &g, bxl.vid, bxl.n_videos, video_loss, st));
    step_mark(3, st);
    RC(echr_stream_join(stream));          // the decoder backward's asynchronous tail: every gradient is final in `stream` order now
    if (x && a->g_tap) {
        // 'CH' / 'CC+CH': d tap_feats gains the attended rows' gradient (the tap columns of the row source), from what the backward left
        echr_row_grad_args r;
        r.col0 = x->clip_parts == 3 ? Dc : 0; r.ncols = a->Ht; r.out = a->g_tap; r.ld = a->Ht; r.ws = ws + L.row_grad;
        RC(row_grad(&d, &g, &r, st, bx != nullptr));          // (a batch: the scatter reads the compacted row list itself, clipctx.hip)
    }
    if (vh && bx) {
        // a batch: video v's scene vector is the mean over ITS rows -- d tap[r, :] += d video[v, vh span] / T_v for r in [row_offset[v], row_offset[v+1])
        RC(echr_seg_col_mean_bwd(ws + L.g_video + a->vh_offset, a->dec.Dv, row_offset, bxl.n_videos, a->Ht, a->Ht, a->g_tap, stream));
        if (a->w_init && a->init_use_v)          // init_linear's d video reaches each video's own rows the same way
            RC(echr_seg_col_mean_bwd(ws + L.g_video_init + a->vh_offset, a->dec.Dv, row_offset, bxl.n_videos, a->Ht, a->Ht, a->g_tap, stream));
    } else if (vh) {
        // scene context 'VH' = tap.mean(0) (CaptionGenerator.py:95-99): d tap[r, :] += d video[vh span] / rows, for the decoder's d video (final
        // behind the join: it is formed in the LSTM-layer stage on a helper stream) and init_linear's
        RC(echr_col_mean_bwd(ws + L.g_video + a->vh_offset, a->tap_rows, a->Ht, a->Ht, a->g_tap, stream));
        if (a->w_init && a->init_use_v) RC(echr_col_mean_bwd(ws + L.g_video_init + a->vh_offset, a->tap_rows, a->Ht, a->Ht, a->g_tap, stream));
    }
    step_mark(4, st);
    if (a->do_step) {                      // clip_gradient + Adam (misc/utils.py:107-111, train.py:315-317)
        const bool rec = sa.ok && hipEventRecord(sa.pre, st) == hipSuccess;          // (stage-ahead: every helper stream was joined just above)
        RC(echr_clamp_adam_counted(a->flat_p, a->flat_g, a->adam_m, a->adam_v, a->n_flat, a->adam_step, a->lr, a->beta1, a->beta2, a->eps, a->clip, a->adam_applied, stream));
        if (rec) { sa.valid = true; sa.st = st; sa.ws = a->ws; sa.flat_g = a->flat_g; }
        else (void)hipGetLastError();
    }
    step_mark(5, st);
    step_timing_end();
    return 0;
}
