// Internal (C++) interfaces between the translation units of libechr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/echr_hip.h"

namespace echr {

// Optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg).
// Disabled by default: ProfScope is then a no-op.  Events are resolved in echr_prof_read after a stream sync.
enum ProfKind { PROF_GEMM = 0, PROF_ATT_FWD = 1, PROF_ATT_BWD = 2, PROF_ATT_POST = 3, PROF_LSTM = 4, PROF_OTHER = 5, PROF_GEMM_SPLIT = 6, PROF_GEMM_H2 = 7, PROF_PACK = 8, PROF_PERSIST = 9, PROF_SST = 10, PROF_KINDS = 11 };
struct ProfScope {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    ProfScope(int kind, double flops, double bytes, hipStream_t st);
    ~ProfScope();
    int kind; double flops, bytes;
};

// runtime switches (initial values from the environment, changeable through echr_config_set)
struct Config { int gemm_bf16x3; int att_slots; int gemm_h2; int persist; int persist_stamps; int gemm_tile; int gemm_split; int persist_bwd; int persist_h2; int persist_coop; int persist_inject_timeout; int persist_spin_limit; int sst_persist; int diag_skip; int persist_sample; int posemb_rows; int gemm_skinny; int posemb_packed; int pair_tables; int persist_sample_force_eos; int persist_sample_max; int deterministic; int row_grad_list; };
// diag_skip (diagnostic, tools/skip_bounds.py; results are WRONG while a bit is set): 1 = h2 operand packs, 2 = clamp+Adam kernel, 4 = att_post, 16 = every fp32-path product (gemm_f32 / t128 / bf16x3), 32 = every h2 product, 64 / 128 = the h2m16 product kernel loads only / computes only (tools/h2_ablate.py),
// 8 = embedding scatter-add -- the launch is skipped, which bounds what removing / hiding that work could gain
Config& config();

int gemm(const echr_gemm_desc& d, hipStream_t st);
// while one is alive on the calling thread, auto split-K (fp32 atomics, order-dependent last bits) is disabled: every product is a
// single fixed-order k loop per output tile
struct DeterministicScope { DeterministicScope(); ~DeterministicScope(); };
bool deterministic_gemm();
// "deterministic" = 1 (echr_config_set / ECHR_DETERMINISTIC): every order-dependent sum of a training iteration (fp32 atomics: split-K epilogues,
// k-slices of the recurrence products, column sums, scatter-adds, the attention backward's shared rows, the persistent kernels' exchange adds) is
// replaced by a fixed-order one -- two runs on the same inputs then agree bit for bit.  Slower; the persistent recurrence kernels are not used.
inline bool det_mode() { return config().deterministic != 0; }
// scratch slabs of the fixed-order variants: one lazily grown device buffer per use (`kind`), owned by the library, never shrunk; the call
// that grows one synchronises the device (hipFree / hipMalloc).  One calling thread, like the rest of the library's static state.
enum { DET_DQ = 0, DET_DPALL = 1, DET_ALPHA = 2, DET_REC = 3, DET_ROWG = 4, DET_KINDS = 5 };
float* det_scratch(int kind, size_t floats);

// persistent (one launch for all timesteps) recurrence of the decoder, csrc/persist.hip
struct DropCfg;
struct PersistFwdBufs { float* GATES[3]; float* CS[3]; float *HS, *OUTD, *QS, *WT, *ATT, *PALL, *xws; bool prezeroed = false;
                        const float* EVB0 = nullptr; };      // EVB0: event part of stream 0's gates, still to be added (persist_fwd_adds_evb0)
bool persist_fwd_adds_evb0();          // the persistent forward launch can add EVB0 itself (fp16-pair LSTM role)
void persist_fwd_zero_range(const echr_dec_args* a, float* xws, float** ptr, long* count);
long persist_fwd_ws_floats(int S);
bool persist_fwd_eligible(const echr_dec_args* a);
int persist_fwd(const echr_dec_args* a, const PersistFwdBufs& B, const DropCfg& dh, const DropCfg& dout, hipStream_t st);
// The forward attention chain's weight images (fp16-pair B fragments of W_hh1 / W_att / W_h2a with their column scales: parameters only) built
// AHEAD of the launch into the exchange workspace, by a small kernel on `st`; the next persist_fwd on the same workspace copies them into LDS
// (2 x 64 KB per gate workgroup from L2) instead of converting them from the strided weight rows in front of its first step.  No-op (returns 0)
// for shapes / configurations the persistent fp16-pair forward kernels do not take.
int persist_fwd_prebuild(const echr_dec_args* a, float* xws, hipStream_t st);
struct PersistBwdBufs { const float* GATES[3]; const float* CS[3]; const float *QS, *WT, *ATT, *PALL, *DOUT; float* DG[3]; float *DQ, *DSC, *xws; bool prezeroed = false; };
void persist_bwd_zero_range(const echr_dec_args* a, float* xws, float** ptr, long* count);
long persist_bwd_ws_floats(int S);
bool persist_bwd_eligible(const echr_dec_args* a);
int persist_bwd(const echr_dec_args* a, const PersistBwdBufs& B, const DropCfg& dh, const DropCfg& dout, hipStream_t st);
// greedy decoding on the persistent kernels (64 events per launch, every step on device): see PersistS in csrc/persist.hip
struct PersistSampleBufs { float* PALL; const float* EVB0; const float* VIDB; float* xws; const float* TG[3]; const float* limg; float* sws; long long* seq; float* seq_logp; int* n_unfinished;
                           long vidb_ld = 0; };          // vidb_ld: row pitch of VIDB (0: one [4H] vector for every event; 4H: one row per event, multi-video batches)
long persist_sample_ws_floats(int S, int V1);          // per group of 64 events
long persist_sample_x_floats(int S);                   // per group of 64 events
long persist_logit_image_floats(int V1);
bool persist_sample_shape_ok(const echr_dec_args* a);
bool persist_sample_eligible(const echr_dec_args* a);
int persist_logit_image(const float* w_logit, int V1, float* img, hipStream_t st);
int persist_sample(const echr_dec_args* a, const PersistSampleBufs& B, hipStream_t st);
int persist_check_async();
long long persist_take_skipped_updates();          // updates the optimiser kernels skipped under the abort the last -62 reported (cleared by the read)
void coop_refused(const char* who, const char* why);          // one stderr line the first time a cooperative launch is refused
// device word that is non-zero from the moment a persistent launch aborts until the host has reported it (persist_check_async):
// kernels that would apply results (clamp_adam, clamp) skip their update while it is set; nullptr when the state is unavailable
const unsigned* persist_abort_word();
// word of the 256-byte abort block in which the optimiser kernels count the updates they skipped while the abort word was set
constexpr int ABORT_SKIPPED_WORD = 16;
unsigned* persist_host_flag();          // device view of the host-mapped flag persist_check_async reads (nullptr when unavailable)
// words of that host-mapped block (16 x 32 bit) beside word 0, the abort code: the largest |p| / |q| an attention kernel met outside the domain of
// its factored tanh (float bits, 0 = none; persist_check_async reports them as -EDOM), and the soft-max branch the last persistent forward
// launch took (1: no shift, 2: max exchange; read-only diagnostic, echr_persist_softmax_branch)
constexpr int DOMAIN_WORD_P = 1, DOMAIN_WORD_Q = 2, BRANCH_WORD = 3;
int persist_softmax_branch();
// the library's helper stream outside a backward pass (the one the asynchronous decoder-backward tail uses): `aux_fork` makes it continue
// after everything queued on `from` and returns it, `aux_join` makes `to` wait for what was queued on it since
// Flags of every event the library uses to order its own streams on ONE device: no timing, and no system-scope fence -- the default event
// release writes the caches back and invalidates them for the host and other devices, which neither a stream-to-stream edge nor the staging
// ring's "this copy kernel has finished" needs (ECHR_EVENT_SYSTEM_FENCE=1 restores the default)
inline unsigned sync_event_flags() {
    static const unsigned f = [] {
        const char* e = getenv("ECHR_EVENT_SYSTEM_FENCE");
        if (e && e[0] == '1') return (unsigned)hipEventDisableTiming;
        return (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
    }();
    return f;
}
void fork_event(hipEvent_t ev);                  // forks that follow wait for `ev` (the caller's stream's last record) instead of recording their own; nullptr ends it
hipStream_t aux_fork(hipStream_t from);          // nullptr when unavailable
int aux_join(hipStream_t to);
hipStream_t aux2_fork(hipStream_t from);         // the same on the decoder's prepare stream (idle during a backward pass); nullptr when unavailable
int aux2_join(hipStream_t to);
bool helpers_available();
hipStream_t aux2_stream();
hipStream_t tail_stream_raw();                   // the tail stream itself, NOT ordered behind anything (echr_train_step's stage-ahead form); nullptr when unavailable
int prep_stream_wait(hipEvent_t ev);             // the prepare stream waits for `ev` (in addition to whatever its next fork waits for)
hipStream_t helpers_merge_to_tail();
int tail_publish();
int tsrm_position_early(const echr_tsrm_args* a, hipStream_t from);          // echr_train_step: start the event encoder's position branch right behind the index staging
int tsrm_bwd_parts(const echr_tsrm_args* a, const echr_tsrm_grads* g, const echr_dropout* drop, void* stream, int part);
int decoder_bwd_scratch_ahead(const echr_dec_args* a, const echr_dec_grads* g);
// What a decoder call carries beside its argument structs.  A default-constructed value is a single video, the plain criterion and no hand-over.
//   bx: the multi-video batch extension (echr_batch_ext, below); scene_rows: the per-video scene part of stream 2's gates is formed with the
//   single-video entry's own arithmetic (row_matvec per video) instead of one product over the V scene vectors, so a row decodes as it does alone
//   to the bit (echr_decoder_sample_train_batch: a last-bit difference in a logit can flip a draw)
//   rw: RewardCriterion's signed weight [N,S] in place of the NLL's mask in the criterion's numerator (echr_train_step_rw)
//   handover (+ cb, user): this backward pass records the data-parallel hand-over events (echr_train_step_args.handover, decoder.hip)
struct DecCall {
    const echr_batch_ext* bx = nullptr; bool scene_rows = false;
    const float* rw = nullptr;
    bool handover = false; echr_handover_fn handover_cb = nullptr; void* handover_user = nullptr;
};
int decoder_bwd_parts(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream, int part, const DecCall& c);
// echr_decoder_bwd as that call: the entry checks, then the whole backward pass
int decoder_bwd_checked(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream, const DecCall& c);
void handover_clear();                   // the hand-over points an earlier backward pass recorded are void from here on (echr_handover_wait returns 1)
// echr_decoder_fwd_prepare / echr_tsrm_fwd as echr_train_step calls them: vid (optional) makes the event encoder's softmax block-diagonal
int decoder_fwd_prepare(const echr_dec_args* a, const DecCall& c, void* stream);
int tsrm_fwd_checked(const echr_tsrm_args* a, const echr_dropout* drop, void* stream, const int* vid);
// clip contexts 'CH' / 'CC+CH' (clipctx.hip): the decoder backward's d gates1 and d P_all, the forward's attention weights WT [S,N,A]
void decoder_bwd_views(const echr_dec_args* a, const echr_dec_grads* g, const float** dg1, const float** dpall);
const float* decoder_fwd_wt(const echr_dec_args* a);
int check_dims_public(const echr_dec_args* a, const char* who);
// the frame-level attention launches of decoder.hip for the one-stream decoder (sat.hip): q as one finished [N, Ha] product without its bias,
// d ATT as one [N, D] buffer; att_post_launch zero-expects DPALL / GAREP / GBREP and ADDS d alpha / d b_alpha to g_alpha / g_balpha
struct AttShape { int N, A, Ha, D; };
DropCfg make_drop(const echr_dropout* d, float p);
int att_check_dims(const AttShape& s, const char* who);
int att_score_launch(const AttShape& s, const float* PALL, const float* Q1, const float* b_q, float* QS, const float* alpha, const float* b_alpha,
                     const int* ev_start, const int* ev_len, float* SC, hipStream_t st);
int att_context_launch(const AttShape& s, const float* C3D, const float* SC, const int* ev_start, const int* ev_len, float* WT, float* ATT, hipStream_t st);
int att_bwd_launch(const AttShape& s, const float* PALL, const float* C3D, const float* Q, const float* alpha, const float* WT, const float* ATT,
                   const float* DATT, const int* ev_start, const int* ev_len, float* DSC, float* DQ, hipStream_t st);
int att_post_replicas();
int att_post_launch(const AttShape& s, int Tv, int S, int rows_disjoint, const float* PALL, const float* QS, const float* alpha, const float* DSC,
                    const int* ev_start, const int* ev_len, float* DPALL, float* GAREP, float* GBREP, float* g_alpha, float* g_balpha, hipStream_t st);
// list_form: the context-term scatter reads the compacted active_rows list itself (echr_train_step_batch_clip; "row_grad_list" = 0 or a step count
// beyond its LDS flags: the flag form every other entry launches)
int row_grad(const echr_dec_args* a, const echr_dec_grads* g, const echr_row_grad_args* r, hipStream_t st, bool list_form = false);
int clip_rows(const float* c3d, int Dc, const float* tap, int Ht, float* rows, int Tv, hipStream_t st);
int join_tail(hipStream_t st);          // make st wait for an asynchronous decoder-backward tail (decoder.hip); no-op when none is pending
int persist_read_stamps(unsigned long long* dst, int max_entries);
unsigned long long* persist_stamp_buffer(int S, hipStream_t st);      // diagnostic: [4][S <= 256][16] stamps, zeroed on st (nullptr: unavailable)
int gemm_grouped(const echr_gemm_desc* ds, int ng, hipStream_t st);
// C[M, Nc <= 16] = A[M, K] . W[Nc, K]^T + bias for very tall A (a stream over A; exact fp32 MFMA, plain stores)
bool gemm_skinny_ok(int M, int Nc, int K, long lda, long ldw, const float* A, const float* W);
int gemm_skinny_nt(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, int M, int Nc, int K, hipStream_t st);
// h2-packed operands (csrc/gemm.hip: two block-scaled fp16 planes): bytes of the packed image of a [rows x cols] operand (cols =
// contraction axis), the packing pass, and a multi-operand packing launch
struct H2PackJob { const float* src; unsigned char* dst; int R, K; long s_row, s_col;
                   const int* gather = nullptr; };      // optional: source row i (the strided axis: operand rows of a row pack, k of a transposing one) is read from row gather[i]
long h2_bytes(int rows, int cols);
int h2_pack(const float* src, int rows, int cols, long s_row, long s_col, void* dst, hipStream_t st);
int h2_pack_multi(const H2PackJob* jobs, int n, hipStream_t st);
inline long h2_floats(int rows, int cols) { return (h2_bytes(rows, cols) + 3) / 4; }
// packed operand of the rows x K matrix stored k-contiguous with leading dimension ld ...
inline H2PackJob pack_rows(const float* src, long ld, int rows, int K, float* dst) {
    return H2PackJob{src, reinterpret_cast<unsigned char*>(dst), rows, K, ld, 1};
}
// ... or stored transposed: element (r, k) at src[k * ld + r]
inline H2PackJob pack_cols(const float* src, long ld, int rows, int K, float* dst) {
    return H2PackJob{src, reinterpret_cast<unsigned char*>(dst), rows, K, 1, ld};
}


// C[M,N] = A[M,K] . W[N,K]^T  (nn.Linear forward; row-major operands with leading dimensions)
inline echr_gemm_desc desc_nt(const float* A, long lda, const float* W, long ldw, float* C, long ldc, int M, int N, int K) {
    echr_gemm_desc d{};
    d.A = A; d.B = W; d.C = C; d.M = M; d.N = N; d.K = K;
    d.sam = lda; d.sak = 1; d.sbk = 1; d.sbn = ldw; d.ldc = ldc;
    d.batch = 1; d.alpha = 1.f; d.beta = 0.f; d.split_k = 1;
    return d;
}
// C[M,N] = A[M,K] . B[K,N]   (data gradient dX = dY . W)
inline echr_gemm_desc desc_nn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
    echr_gemm_desc d = desc_nt(A, lda, B, 1, C, ldc, M, N, K);
    d.sbk = ldb; d.sbn = 1;
    return d;
}
// C[M,N] = A[K,M]^T . B[K,N] (weight gradient dW = dY^T . X)
inline echr_gemm_desc desc_tn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
    echr_gemm_desc d = desc_nn(A, 1, B, ldb, C, ldc, M, N, K);
    d.sam = 1; d.sak = lda;
    return d;
}

// C[M,N] = A . B^T on two h2-packed operands
inline echr_gemm_desc desc_h2(const float* Apk, const float* Bpk, float* C, long ldc, int M, int N, int K) {
    echr_gemm_desc d = desc_nt(Apk, K, Bpk, K, C, ldc, M, N, K);
    d.split_k = -1; d.algo = ECHR_GEMM_H2;
    return d;
}

// column sums: out[j] (+)= sum_i X[i*ld + j], i < rows
int colsum(const float* X, long ld, int rows, int cols, float* out, bool accumulate, hipStream_t st);
int colsum2(const float* X, long ld, int rows, int cols, float* out, float* out2, bool accumulate, hipStream_t st);
// several accumulating column sums in one launch (out / out2 / out3 += column sums of X; out2, out3 optional)
constexpr int COLSUM_MAX_JOBS = 8;
struct ColsumJob { const float* X; long ld; int rows, cols; float* out; float* out2; float* out3; };
int colsum_multi(const ColsumJob* jobs, int n, hipStream_t st);
// out[n*ld_out + j] = sum_t X[(t*N + n)*ld + j]
int sum_over_time(const float* X, long ld, int S, int N, int cols, float* out, long ld_out, hipStream_t st);
int fill_zero(float* p, long n, hipStream_t st);
int fill_zero_2d(float* p, int rows, int cols, long ld, hipStream_t st);
constexpr int FILL_MAX_JOBS = 8;
int fill_zero_multi(float* const* ptrs, const long* counts, int n, hipStream_t st);     // several ranges, one launch
constexpr int TRANSPOSE_MAX_JOBS = 8;
struct TransposeJob { const float* in; long ld_in; float* out; long ld_out; int rows, cols; };
int transpose_multi(const TransposeJob* jobs, int n, hipStream_t st);                    // several out[c,r] = in[r,c], one launch
// out[c, r] = in[r, c] for r < rows, c < cols; rows..rows_pad-1 of the output's row are zero-filled (k padding)
int transpose(const float* in, long ld_in, float* out, long ld_out, int rows, int cols, int rows_pad, hipStream_t st);
int embed_gather(const float* W, const int* tok, float* out, int rows, int E, int V1, hipStream_t st);
int row_matvec(const float* x, const float* W, long ldw, const float* b1, const float* b2, float* out, int N, int K, hipStream_t st);
// row_matvec for M vectors x [M, ldx] -> out [M, ldo] in one launch (row_matvec is its M = 1 case: a row is bit-identical alone and among M)
int rows_matvec(const float* x, long ldx, const float* W, long ldw, const float* b1, const float* b2, float* out, long ldo, int M, int N, int K, hipStream_t st);
int rank1_update(const float* x, const float* y, float* C, long ldc, int M, int N, bool accumulate, hipStream_t st);
int vec_mat(const float* x, const float* W, long ldw, float* out, int M, int N, hipStream_t st);
int embed_scatter_add(const float* dX, const int* tok, float* gW, int rows, int E, int V1, hipStream_t st, const int* rowmap = nullptr);
int logsoftmax_rows(float* X, long ld, int N, int S, int t0, int nt, int cols, hipStream_t st);
int logsoftmax_bwd(const float* logp, const float* G, const void* target, int tgt64, const float* mask, const float* g_loss,
                   const float* mask_sum, float* out, long ldo, int N, int S, int V1, hipStream_t st, const float* rw = nullptr, bool unit_den = false);
// log-softmax + masked NLL + d logits in one pass over the logits (echr_train_step); rows_sum turns the per-row terms into (loss, sum(mask))
bool logsoftmax_nll_dlg_ok(int V1, long ldo);
int logsoftmax_nll_dlg(const float* X, long ld, const void* target, int tgt64, const float* mask, const float* g_loss, float* out, long ldo,
                       float* row_loss, float* msum_out, int N, int S, int V1, hipStream_t st, const int* act = nullptr, int n_active = 0,
                       const float* rw = nullptr, bool unit_den = false);
int nll_rows_sum(const float* row_loss, int NS, const float* msum, float* loss, hipStream_t st, bool rw = false, bool unit_den = false);
// RewardCriterion's loss from log-probs [N,S,V1]: out = (sum(-logp[target] * rw) / sum(mask), sum(mask))
int nll_loss_rw(const float* logp, const void* target, int tgt64, const float* mask, const float* rw, float* loss, int N, int S, int V1, hipStream_t st, bool unit_den);

// Multi-video batches (echr_batch_ext, include/echr_hip.h).  The extension is an argument of every internal function that needs it -- the
// *_batch entry points and echr_train_step_batch* hand it down (DecCall.bx, `vid`, `unit_den`), every single-video entry passes nullptr -- so
// what a function does is decided by what it is called with:
//   event encoder: block-diagonal softmax by vid; decoder: per-row scene part of stream 2's gates and its segmented gradients;
//   criterion: the weighted (rw) form with denominator 1 (unit_den) -- the per-video normalisers sum(mask_v) + 1e-6 arrive inside the weights
// out[v*ld + c] = sum over the rows n with vid[n] == v of X[n*ld + c], rows added in ascending n (fixed order: bit-reproducible)
int seg_rowsum(const float* X, const int* vid, int N, int V, int cols, long ld, float* out, hipStream_t st);
// per-video losses of a batch: vloss[v] = sum of row_loss over the rows of video v (row i is the time-major row act[i], or i itself) ...
int video_loss_rows(const float* row_loss, const int* act, int rows, int N, const int* vid, int V, float* vloss, hipStream_t st);
// ... or from log-probs [N,S,V1]: vloss[v] = sum over the events n of video v and t of -logp[n,t,target[n,t]] * w[n,t]
int video_loss_logp(const float* logp, const void* target, int tgt64, const float* w, int N, int S, int V1, const int* vid, int V, float* vloss, hipStream_t st);
int decoder_fused_video_loss(const echr_dec_args* a, const echr_dec_grads* g, const int* vid, int V, float* vloss, hipStream_t st);

// echr_decoder_fwd with the criterion fused behind the logits product: g carries nll_target / nll_mask / g_loss / ws_bwd; d logits land in ws_bwd
// (echr_dec_grads.dlg_ready = 1 for the echr_decoder_bwd that follows); returns through *fused whether the fused form applied
// (g = fused = compact = nullptr: echr_decoder_fwd itself, as the call `c`)
int decoder_fwd_fused(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream, bool* fused, bool* compact,
                      const DecCall& c);
int decoder_fused_loss(const echr_dec_args* a, const echr_dec_grads* g, float* loss, hipStream_t st, bool rw, bool unit_den);
int sample_step(const float* logits, long ld, int N, int V1, int t, int seq_len, int* it_next, int* unfinished, long long* seq,
                float* seq_logp, int* n_unfinished, float temperature, unsigned long long seed, hipStream_t st);
// the multinomial step with the row on chip (echr_decoder_sample_train_batch): sample_step's draw, bit for bit, with the slab sum folded in
// (slabs != nullptr: the row is formed from the k-slice slabs + bias; else read from `logits`); V1 floats of LDS up to 12 288 words
int sample_row_step(float* logits, long ld, int N, int V1, int t, int seq_len, int* it_next, int* unfinished, long long* seq, float* seq_logp,
                    int* n_unfinished, float temperature, unsigned long long seed, hipStream_t st, const float* slabs, long slab_stride,
                    const float* bias, int nslab);
// video_words [V+1] = per-video maxima of the rows' non-zero token counts in seq [N,L] (vid per row, non-decreasing), then the maximum of all
int sample_video_words(const long long* seq, const int* vid, int N, int L, int V, int* video_words, hipStream_t st);
// slabs != nullptr: logits rows are formed here from four k-slice slabs (+ bias) in a fixed order and written to `logits`
int greedy_step(float* logits, long ld, int N, int V1, int t, int seq_len, int* it_next, int* unfinished,
                long long* seq, float* seq_logp, int* n_unfinished, hipStream_t st, const float* slabs = nullptr, long slab_stride = 0,
                const float* bias = nullptr, int nslab = 0);
// beam search (beam.hip; driver echr_decoder_beam in decoder.hip): per-slot scores / alive flags and histories [rows, L], per-event result
struct BeamState { float* SCORE; int* ALIVE; int* HTOK; float* HLP; int* BTOK; float* BLP; float* BSCORE; int* BW; };
int beam_step(const float* logits, int V1, int E, int B, int t, int L, int* IT, const BeamState& bs, float* HS, float* C0, float* C1, float* C2,
              int H, hipStream_t st);
int beam_finalize(const BeamState& bs, int E, int L, long long* seq, float* seq_logp, float* score, int* words, hipStream_t st);
// echr_decoder_beam_batch: video_words [V+1] = per-video maxima of words [E] (vid per row, B rows per event), then the maximum of all
int beam_video_words(const int* words, const int* vid, int E, int B, int V, int* video_words, hipStream_t st);

}  // namespace echr
