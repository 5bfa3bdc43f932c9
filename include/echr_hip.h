/*
 * echr_hip.h -- C ABI of libechr_hip.so: the MI355X (gfx950) implementation of ECHR's
 * hierarchical-encoder + attention caption-decoder hot path.
 *
 * The reference (ttengwang/ECHR) has no FFI layer of its own: its boundary is the Python module API
 * (CaptionGenerator.py:17, models/__init__.py:6-29).  echr_amd/ keeps that Python API and calls the
 * entry points below through ctypes; each entry point names the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a BORROWED device pointer (PyTorch owns all memory; the library never
 *    allocates or frees user-visible buffers); tensors are row-major contiguous fp32 unless a
 *    leading dimension is given; index tensors are int32.
 *  - `stream` is a hipStream_t passed as void*; calls are asynchronous w.r.t. the host, re-entrant,
 *    never synchronise, and are legal inside hipGraph stream capture.
 *  - return 0 on success, negative errno-style code on failure; echr_last_error() returns the
 *    calling thread's last message.
 */
#ifndef ECHR_HIP_H
#define ECHR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): echr_train_step_args.handover, echr_handover_wait, echr_async_skipped_updates; round 4 had grown the decoder's
 * argument struct (train, zero_extra, zero_extra_count) and its gradient struct (dlg_ready, active_rows, n_active) under version 1.  A binding that restates
 * the structs MUST also compare its sizeof() of each with echr_abi_sizeof(): the version alone does not describe the layouts. */
/* 3 (round 6): echr_clamp_adam_counted, echr_train_step_args.adam_applied (a per-optimiser count of APPLIED updates; the process-wide
 * echr_async_skipped_updates now counts echr_clamp_adam launches only); echr_train_step_args.event_parts / w_init.. / vh_offset: the
 * reference's 'ER1' / 'ER2' event contexts, CG_init_feats_type and the 'VH' scene context's gradient on the one-call path. */
#define ECHR_ABI_VERSION 3

int echr_version(void);
/* sizeof() of an argument struct of this header by its type name ("echr_dec_args", ...), -1 for an unknown name: lets a binding that
 * restates the structs (ctypes, cgo, JNI) check its layout against the library it loaded */
int64_t echr_abi_sizeof(const char* name);
const char* echr_last_error(void);
/* Asynchronous failures.  The persistent recurrence kernels (csrc/persist.hip) bound every inter-workgroup wait; when one gives up the
 * launch drains, a device word stays set (echr_clamp_adam / echr_clamp then skip their update, so no parameter is touched by the
 * invalid gradients) and the NEXT library call that takes a stream returns -ETIME (-62) once, naming the edge and timestep.
 * echr_check_async() is that check on its own, for callers that want it right after a synchronisation point: 0, -62 or -33.
 * -EDOM (-33), reported the same way (once, by the next library call that checks): an attention kernel that evaluates tanh(p + q) in its
 * factored form 1 - 2 / (e^{2p} e^{2q} + 1) (the persistent recurrences, the greedy decoder, the d P_all pass of every backward) met
 * |p| > 43 (p = ctx2att(clip), tensor P_all) or |q| > 43 (q = h2att(h1)): outside that range the form is not tanh(p + q).  Nothing is aborted
 * or skipped -- the launch ran to its end -- but the results of the calls since the last check are invalid; the message names the tensor and
 * the magnitude reached.  The launch-per-phase forward (echr_config_set("persist", 0)) evaluates tanh(p + q) directly and has no such limit. */
int echr_check_async(void);
/* Diagnostic: the soft-max branch the last persistent forward / decoding launch took -- 1: no shift (sum|alpha| <= 40), 2: the exact max
 * exchange between the three workgroups of an event, 0: none yet.  Read it behind a synchronisation point. */
int echr_persist_softmax_branch(void);
/* Number of echr_clamp_adam launches (of ANY optimiser state of the process; echr_clamp is not an update and is not counted) that skipped
 * their update because of the asynchronous failure the last -62 reported (read once: the count is cleared).  Process-wide, therefore only
 * a diagnostic when several optimiser states step in one process: a caller that keeps step counts winds each of them back from its OWN
 * count of applied updates (echr_clamp_adam_counted / echr_train_step_args.adam_applied). */
int64_t echr_async_skipped_updates(void);

/* ------------------------------------------------------------------------------------------------
 * Dense fp32 projection on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain).
 * Replaces every nn.Linear / torch.bmm / addmm site of the path.
 *   C[b][rowmap(i)][j] = act( alpha * sum_k A[b](i,k) * B[b](k,j) + beta * C_old + bias[j] + bias2[j]
 *                             + addend[(i % add_mod)][j] )
 * A(i,k) = A[i*sam + k*sak], B(k,j) = B[k*sbk + j*sbn]; in each pair one stride must be 1.
 * split_k > 1: partial sums are atomically added into C (which must already hold its base value);
 *              act must be ECHR_ACT_NONE and beta is ignored.
 * ---------------------------------------------------------------------------------------------- */
enum { ECHR_GEMM_F32 = 0, ECHR_GEMM_BF16X3 = 1, ECHR_GEMM_H2 = 2 };
enum { ECHR_ACT_NONE = 0, ECHR_ACT_TANH = 1, ECHR_ACT_MUL_DTANH = 2 /* acc * (1 - aux^2) */ };

typedef struct {
    const float* A;
    const float* B;
    float* C;
    int32_t M, N, K;
    int64_t sam, sak, sbk, sbn, ldc;
    int32_t batch;
    int64_t bsa, bsb, bsc;
    float alpha, beta;
    const float* bias;
    int64_t bs_bias;
    const float* bias2;
    const float* addend;
    int32_t add_mod;
    int64_t ld_add;
    int32_t act;
    const float* aux;
    int64_t ld_aux;
    int32_t rowmap_mod, rowmap_mul; /* out row = (i % mod) * mul + i / mod ; mod = 0 -> identity */
    int32_t split_k;
    int32_t algo; /* ECHR_GEMM_F32 (exact v_mfma_f32_32x32x2_f32) or ECHR_GEMM_BF16X3 (fp32 operands split exactly into three
                     bf16 planes, six plane products on v_mfma_f32_32x32x16_bf16, fp32 accumulate: fp32-accurate, 2.7x the rate;
                     needs both operands k-contiguous and 16-byte aligned, else the library silently uses ECHR_GEMM_F32),
                     or ECHR_GEMM_H2: A and B point at operands that echr_h2_pack has already rewritten as two block-scaled fp16
                     planes (below); three fp16 MFMA products per k block, fp32-grade accuracy at 5x the fp32 MFMA rate and
                     fp32's byte count (strides are ignored; batch = 1, no activation) */
    const int32_t* row_index; /* optional output-row scatter: row i of the product is ADDED (fp32 atomics; several rows may share a target) into
                                 C[clamp(row_index[i], 0, row_index_max)] -- the token-embedding gradient d E[tok] += d X[row] without a
                                 materialised d X and a scatter pass (OldModel_NEW.py:110 backward).  Needs beta = 1, act = NONE, no rowmap */
    int32_t row_index_max;
} echr_gemm_desc;

int echr_gemm_f32(const echr_gemm_desc* d, void* stream);
/* Test-facing entries of internal launch forms (tests/test_gpu_gemm_contract.py); the product path calls them inside the library.
 * echr_gemm_grouped: ds[0..n-1], 1 <= n <= 8 problems in ONE launch.  Every problem has batch = 1 and act = NONE, and all of them share K, sam / sak,
 * which of sbk / sbn is 1, alpha, beta, split_k, algo, rowmap_mod, add_mod and ld_add; M and N are shared too unless every problem is
 * ECHR_GEMM_H2 (h2 problems may differ in M and N).  A, B, C, sbk / sbn, ldc, bias, bias2 and addend are per problem.  Problems may share
 * C only in accumulate mode: split_k = -1, beta = 1, K > 32 (they add with fp32 atomics; under echr_config_set("deterministic", 1) they run
 * one after the other instead, bit-identical run to run). */
int echr_gemm_grouped(const echr_gemm_desc* ds, int32_t n, void* stream);
/* echr_gemm_skinny_nt: C[M, Nc] = A[M, K] . W[Nc, K]^T + bias (bias may be null) as one stream over a very tall A.  Requires M >= 4096,
 * 1 <= Nc <= 16, K = 256 or 512, lda % 4 == 0, ldw % 4 == 0, A and W 16-byte aligned, and the "gemm_skinny" switch on; anything else
 * returns -22. */
int echr_gemm_skinny_nt(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc, int32_t M, int32_t Nc,
                        int32_t K, void* stream);

/* h2 operands: a logical [rows x cols] fp32 operand (cols = the contraction axis) rewritten as two fp16 planes with one shared
 * power-of-two scale per row and 256-wide k segment (8 blocks of 32): xs = x * 2^(14 - floor(log2 blockmax)), h1 = fp16(xs), h2 = fp16(xs - h1).
 * No value is held in fp16 unscaled, so the fp32 exponent range survives; h1 + h2 carries 22..24 significand bits of every
 * element within 2^-17 of its segment maximum.  Laid out as zero-padded 128 x 32 chunks in the order the GEMM's direct-to-LDS
 * loads consume.  Element (r, k) is read from src[r*s_row + k*s_col] (one stride must be 1, so a transposed source packs
 * without a separate transpose).  dst: echr_h2_bytes(rows, cols) bytes, 16-byte aligned. */
int64_t echr_h2_bytes(int32_t rows, int32_t cols);
int echr_h2_pack(const float* src, int32_t rows, int32_t cols, int64_t s_row, int64_t s_col, void* dst, void* stream);
/* The same with a gathered strided axis (test-facing entry of the packs the decoder issues over token rows): index i of the axis whose stride
 * is NOT 1 -- operand rows when s_col == 1, k when s_row == 1 -- is read from gather[i] (rows resp. cols device int32 entries, each a
 * valid index of the source; entries may repeat). */
int echr_h2_pack_gather(const float* src, int32_t rows, int32_t cols, int64_t s_row, int64_t s_col, const int32_t* gather, void* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dropout configuration shared by all training-mode entry points (counter-based Philox-4x32-10;
 * bit-identical host implementation: echr_amd/philox.py).  Sites: reference nn.Dropout instances at
 * models/MA_attention_8_NEW.py:162 (p=0.3), models/OldModel_NEW.py:810,814,818 (p=0.5), :136 (CG_drop_prob).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t seed;
    uint32_t offset;   /* forward-call counter */
    int32_t training;  /* 0: every dropout is the identity */
    float p_tsrm, p_h, p_out;
} echr_dropout;

/* ------------------------------------------------------------------------------------------------
 * Event-level context inputs: mean-pool of each event's C3D rows + gather of the proposal-LSTM
 * state at the event's anchor.  Replaces CaptionGenerator.py:111-114,121,128.
 *   ech[n, 0:D]     = mean(c3d[ev_start[n] : ev_start[n]+ev_len[n], :])
 *   ech[n, D:D+Ht]  = tap[ind[n], :]
 * bwd scatters d_ech[:, D:] into d_tap rows (atomic add; d_tap pre-zeroed) -- gradients to c3d are
 * not produced (features are data).
 * ---------------------------------------------------------------------------------------------- */
int echr_event_pool_gather_fwd(const float* c3d, const float* tap, const int32_t* ev_start, const int32_t* ev_len,
                               const int32_t* ind, float* ech, int32_t N, int32_t D, int32_t Ht, void* stream);
int echr_event_pool_gather_bwd(const float* d_ech, const int32_t* ind, float* d_tap, int32_t N, int32_t D, int32_t Ht,
                               void* stream);
/* Non-zero initial decoder state (OldModel.init_hidden, OldModel_NEW.py:72-96; CG_init_feats_type from 'V', 'E', 'C'):
 *   feats = cat([video broadcast over the N events | event | clip.mean(1)], 1);   h0 = init_linear(feats)   [N, 3H]
 * `clip.mean(1)` is the mean over the A PADDED slots of CaptionGenerator.get_clip_context (zeros behind an event's end): sum over the event's
 * rows / A.  bwd: gradients of init_linear (written, or accumulated when `zeroed`), d video (written), d event (ADDED to g_event); c3d is data. */
typedef struct {
    int32_t N, Dv, De, D, H3;                  /* events; widths of the scene / event context, of a C3D row; 3 * rnn_size */
    int32_t use_v, use_e, use_c;               /* 'V' / 'E' / 'C' in CG_init_feats_type */
    int32_t A;                                 /* padded clip length (max event length of the batch) */
    const float *video, *event, *c3d;          /* [Dv], [N,De], [Tv,D] */
    const int32_t *ev_start, *ev_len;
    const float *w, *b;                        /* init_linear.weight [H3, Dtot], .bias [H3] */
    float* feats;                              /* [N, Dtot] scratch; the backward pass reads it again */
    float* h0;                                 /* out [N, H3] */
} echr_init_state_args;
typedef struct {
    const float* g_h0;                         /* [N, H3] */
    float *g_w, *g_b;                          /* [H3, Dtot], [H3] */
    float *g_video, *g_event;                  /* [Dv] written (NULL: not wanted), [N,De] added into (NULL: not wanted) */
    float* dfeats;                             /* [N, Dtot] scratch */
    int32_t zeroed;                            /* 1: g_w / g_b are pre-zeroed accumulation targets */
} echr_init_state_grads;
int echr_init_state_fwd(const echr_init_state_args* a, void* stream);
int echr_init_state_bwd(const echr_init_state_args* a, const echr_init_state_grads* g, void* stream);

/* Scene context 'VC' / 'VH' (CaptionGenerator.get_video_context, CaptionGenerator.py:95-99: `c3d_feats.mean(0)`, `tap_feats.mean(0)`):
 * out[c] = mean over the `rows` rows of x[:, c] (x row-major with leading dimension ld); bwd: gx[r, c] += g[c] / rows. */
int echr_col_mean_fwd(const float* x, int32_t rows, int32_t cols, int64_t ld, float* out, void* stream);
int echr_col_mean_bwd(const float* g, int32_t rows, int32_t cols, int64_t ld, float* gx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TSRM event-relation encoder.  Replaces MA_Attention8.forward (MA_attention_8_NEW.py:35-49) and
 * attention_module_multi_head.forward (:101-177), fST0 / use_posit=1.
 * Parameter pointers use the reference state_dict names (fusion_model.*).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t N, Din, Df, Do, G;
    /* parameters */
    const float *w_emb, *b_emb;      /* event_emb      [Df,Din],[Df] */
    const float *w_fc1, *b_fc1;      /* pair_pos_fc1   [Df,Df],[Df]  */
    const float *w_fc2, *b_fc2;      /* pair_pos_fc2   [G,Df],[G]    */
    const float *w_q, *b_q;          /* query_1        [Df,Df],[Df]  */
    const float *w_k, *b_k;          /* key_1          [Df,Df],[Df]  */
    const float *w_out, *b_out;      /* linear_out_1   [Do,Df(,1,1)],[Do] */
    /* inputs */
    const float* ech;                /* [N,Din] */
    const int32_t *ev_start, *ev_len;
    /* saved activations (caller-allocated; sizes via echr_tsrm_ws_floats) */
    float* ws;
    /* output */
    float* out;                      /* [N,Do] */
    int32_t inference;               /* echr_tsrm_fwd: 1 = no echr_tsrm_bwd will follow on this workspace (activations that only the backward
                                        pass reads -- the fp32 position embedding of >= 4096 pairs -- are not materialised) */
    int32_t max_len, max_span;       /* optional, known to the host from the index lists: max ev_len and max |(2 start_i + len_i) - (2 start_j +
                                        len_j)| over the events (0 / -1... leave max_len = 0 when unknown).  With `inference` and >= 16384 pairs
                                        they let the pair MLP run from tables over the distinct (|2 dc|, l_i) and (l_i, l_j) keys */
    int32_t fst_mode;                /* how position gate and scaled affinity combine ahead of the softmax (MA_attention_8_NEW.py:148-157):
                                        0 = fST0 gate * aff (the recipe), 1 = fST1 gate + aff, 2 = fST2 log(clamp(gate, 1e-6)) + aff,
                                        3 = fST3 the gate alone, 4 = use_posit = 0: the affinity alone (the position branch is not run and
                                        pair_pos_fc1 / fc2 receive no gradient) */
} echr_tsrm_args;

typedef struct {
    /* parameter gradients (written, not accumulated, unless `zeroed`) */
    float *g_w_emb, *g_b_emb, *g_w_fc1, *g_b_fc1, *g_w_fc2, *g_b_fc2, *g_w_q, *g_b_q, *g_w_k, *g_b_k, *g_w_out, *g_b_out;
    float* g_ech;                    /* [N,Din] */
    const float* g_out;              /* [N,Do] */
    float* ws_bwd;                   /* scratch, echr_tsrm_ws_bwd_floats */
    int32_t zeroed;                  /* 1: the caller zero-filled every parameter-gradient buffer (flat arena): the
                                        library accumulates into them and skips its own zero fills */
} echr_tsrm_grads;

int64_t echr_tsrm_ws_floats(int32_t N, int32_t Din, int32_t Df, int32_t Do, int32_t G);
int64_t echr_tsrm_ws_bwd_floats(int32_t N, int32_t Din, int32_t Df, int32_t Do, int32_t G);
int echr_tsrm_fwd(const echr_tsrm_args* a, const echr_dropout* drop, void* stream);
int echr_tsrm_bwd(const echr_tsrm_args* a, const echr_tsrm_grads* g, const echr_dropout* drop, void* stream);
/* attention_module_multi_head.forward on its own (MA_attention_8_NEW.py:101-177, fST0, use_posit = 1): roi_feat [N,Df] = the embedded
 * events, pos_emb [N,N,Df] = the pairwise position embedding; a->ech / ev_start / ev_len / w_emb / b_emb are not read (Din only
 * sizes the workspace).  Forward only. */
int echr_tsrm_attn_fwd(const echr_tsrm_args* a, const float* roi_feat, const float* pos_emb, const echr_dropout* drop, void* stream);
/* position embedding alone (float64 math on device, fp32 result [N,N,Df]); replaces the numpy
 * extract_position_matrix / extract_position_embedding (:51-79) + the host->device copy at :41 */
int echr_tsrm_posemb(const int32_t* ev_start, const int32_t* ev_len, float* pos, int32_t N, int32_t Df, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Three-stream attention caption decoder.  Replaces OldModel.forward (teacher forcing,
 * models/OldModel_NEW.py:98-130), get_logprobs_state (:133-137), ThreeStream_Core.forward (:801-823),
 * Attention.forward (:376-401), the greedy branch of OldModel.sample (:139-187), and, optionally
 * fused, LanguageModelCriterion (misc/utils.py:66-75).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t N, A, Tv, D, H, E, Ha, De, Dv, V1, S;
    int32_t rows_disjoint;                     /* 1: no two events share a video row (lets d P_all be stored instead of atomically added) */
    /* parameters (reference state_dict names under lm_model.) */
    const float* embed;                        /* embed.weight [V1,E] */
    const float *w_logit, *b_logit;            /* logit [V1,3H],[V1] */
    const float* w_ih[3];                      /* core.layer{k}.weight_ih [4H, E+ctx_k] */
    const float* w_hh[3];                      /* [4H,H] */
    const float* b_ih[3];
    const float* b_hh[3];
    const float *w_c2a, *b_c2a;                /* core.attention.ctx2att [Ha,D],[Ha] */
    const float *w_h2a, *b_h2a;                /* h2att [Ha,H],[Ha] */
    const float *w_alpha, *b_alpha;            /* alpha_net [1,Ha],[1] */
    /* inputs */
    const float* c3d;                          /* [Tv,D] */
    const int32_t *ev_start, *ev_len;          /* [N] (clip context = rows ev_start..ev_start+ev_len) */
    const float* event;                        /* [N,De] */
    const float* video;                        /* [Dv]   */
    const int32_t* tokens;                     /* [S,N] time-major input tokens (labels[:, t]) */
    /* workspace (saved for backward), echr_decoder_ws_floats */
    float* ws;
    /* output: log-probs [N,S,V1] */
    float* logp;
    int32_t prepared;                          /* echr_decoder_fwd only: 1 = echr_decoder_fwd_prepare already ran on this workspace */
    int32_t train;                             /* 1 = echr_decoder_bwd will follow on this workspace: what only the backward pass reads and depends on
                                                  parameters alone (the transposed h2 image of W_logit for d OUTD = d logits . W_logit) is packed by the
                                                  forward's own packing launch, off the critical path in front of the reverse recurrence.  Pass the
                                                  SAME value to echr_decoder_fwd_prepare / echr_decoder_fwd / echr_decoder_bwd.  0: the backward packs it */
    float* zero_extra;                         /* echr_decoder_fwd / _prepare, optional: a range the caller wants zero-filled before the backward pass (its
                                                  gradient arena), folded into the forward's first fill launch; NULL = none */
    int64_t zero_extra_count;                  /* floats */
    const float* h0;                           /* optional [N, 3H]: the initial state, `init_linear(cat(...))` BEFORE its view / transpose
                                                  (OldModel_NEW.py:72-96, CG_init_feats_type non-empty): stream k starts from h = c = h0[:, kH:(k+1)H].
                                                  NULL = the recipe's zero state.  With it the recurrences run launch per phase (the persistent
                                                  kernels assume h(-1) = 0) */
} echr_dec_args;

typedef struct {
    float* g_embed;                            /* [V1,E] must be zeroed by the caller (scatter-add) */
    float *g_w_logit, *g_b_logit;
    float* g_w_ih[3];
    float* g_w_hh[3];
    float* g_b_ih[3];
    float* g_b_hh[3];
    float *g_w_c2a, *g_b_c2a, *g_w_h2a, *g_b_h2a, *g_w_alpha, *g_b_alpha;
    float* g_event;                            /* [N,De] */
    float* g_video;                            /* [Dv] or NULL */
    const float* g_logp;                       /* [N,S,V1] upstream gradient, or NULL when nll_* are set */
    /* fused criterion path: d loss / d logp = -mask/(sum(mask)+1e-6) * g_loss at the target entries */
    const int32_t* nll_target;                 /* [N,S] or NULL */
    const float* nll_mask;                     /* [N,S] */
    const float* g_loss;                       /* device scalar */
    float* ws_bwd;                             /* scratch, echr_decoder_ws_bwd_floats */
    int32_t zeroed;                            /* 1: parameter-gradient buffers arrive zero-filled (see echr_tsrm_grads) */
    int32_t phase;                             /* 0: the whole backward.  A data-parallel caller may run it in stages ON THE SAME ws_bwd and
                                                  start reducing gradients as they become final:
                                                    1 = late-fusion stage (d logits; g_w_logit, g_b_logit final: 35 % of the bytes),
                                                    3 = reverse recurrence + every gradient of the three LSTM layers (g_w_ih, g_w_hh,
                                                        g_b_ih, g_b_hh, plus g_w_h2a, g_b_h2a, g_event, g_video): 39 % of the bytes,
                                                    4 = the rest (attention parameters, token embedding);
                                                    2 = 3 followed by 4.   1, 3, 4 in this order equal 0. */
    int32_t async_tail;                        /* phase 0 only: 1 = the last stage (attention-parameter and token-embedding gradients; nothing else
                                                  in a backward pass depends on them) runs on a library-owned second stream and the call returns
                                                  without joining it, so that the caller's next backward kernels (event encoder, proposal encoder)
                                                  overlap it; the logit-layer gradients are formed there too.  The caller MUST call
                                                  echr_stream_join(stream) before anything reads g_w_logit, g_b_logit, g_w_c2a,
                                                  g_b_c2a, g_w_alpha, g_b_alpha, g_embed or frees ws / ws_bwd (every library entry that takes a
                                                  stream joins first as a safety net).
                                                  2 = additionally only g_event (and what it needs) is formed on `stream`; every other gradient
                                                  of the three LSTM layers (g_w_ih, g_w_hh, g_b_ih, g_b_hh, g_w_h2a, g_b_h2a, g_video) is formed on
                                                  a second library-owned stream and is final only after echr_stream_join as well (needs zeroed = 1) */
    const float* nll_msum;                     /* fused criterion path, optional: device pointer to sum(nll_mask) (the second output of
                                                  echr_nll_loss_fwd); NULL = the library sums the mask itself */
    float* zero_extra;                         /* optional: a range the caller wants zero-filled before any gradient is written (its gradient
                                                  arena span when `zeroed` = 1): folded into the backward's own multi-range fill launch
                                                  (stage 1) instead of a separate fill; NULL = none */
    int64_t zero_extra_count;                  /* floats */
    int32_t nll_target_i64;                    /* 1: nll_target points at int64 indices (the reference's LongTensor labels as they are: no
                                                  conversion pass), 0: int32 */
    int32_t dlg_ready;                         /* 1: d logits already sit in ws_bwd (echr_train_step forms them in the pass that reads the logits:
                                                  log-softmax + criterion + its gradient in one kernel); callers of echr_decoder_bwd leave it 0 */
    const int32_t* active_rows;                /* echr_train_step only (with dlg_ready): the n_active time-major rows t*N + n with t <= the last
                                                  timestep at which caption n's criterion mask is non-zero, ascending.  Rows outside carry exactly zero
                                                  d logits (misc/utils.py:66-75: the mask multiplies the log-prob) and, as nothing later in the caption
                                                  feeds back into them, exactly zero d gates / d q, so the late-fusion products run on the compacted
                                                  rows (logits and d logits exist as [n_active, V1], d OUTD is scattered back by row, d W_logit contracts
                                                  over n_active rows) and the recurrent weight gradients and d XT contract / run over the same rows */
    int32_t n_active;
    float* g_h0;                               /* optional [N, 3H] out (written): d loss / d h0 = d h(-1) + d c(-1) of every stream (echr_dec_args.h0) */
} echr_dec_grads;

/* make `stream` wait for an asynchronous decoder-backward tail (echr_dec_grads.async_tail); no-op when none is pending */
int echr_stream_join(void* stream);

/* Frame-level contexts 'CH' / 'CC+CH' (CaptionGenerator.py:140-167): the decoder's row source echr_dec_args.c3d is then tap_feats [Tv, Ht]
 * itself ('CH', D = Ht) or the rows [Tv, Dc + Ht] = [c3d | tap] ('CC+CH', echr_clip_rows), and the attention reaches tap_feats.
 * echr_decoder_row_grad runs after echr_decoder_bwd on the same ws / ws_bwd (any phase-0 form, asynchronous tail included: the call orders
 * that tail first) and ADDS the gradient of columns [col0, col0 + ncols) of the row source into out (row r at out + r * ld):
 *   out[start_n + a] += sum_t WT[t,n,a] . (d gates1[t,n] . W_ih1[:, E + col0 + c])  +  (d P_all . W_c2a[:, col0 + c])[start_n + a]
 * for a < len_n, summed over every event that covers the row.  rows_disjoint = 1: plain updates; otherwise atomic adds, or with the
 * "deterministic" configuration per-event slabs folded per row in event order (bit-identical run to run).  out must hold dec.Tv rows.
 * Equally valid behind echr_decoder_bwd_batch on the same ws / ws_bwd (the batch extension changes neither workspace layout; ev_start and
 * dec.Tv are then batch-absolute / T_tot, and a row only ever gains from events of its own video). */
typedef struct {
    int32_t col0;            /* first wanted column of the row source ('CH': 0, 'CC+CH': Dc) */
    int32_t ncols;           /* wanted columns (Ht) */
    float* out;              /* [>= Tv, ld] accumulated into (d tap_feats) */
    int64_t ld;              /* leading dimension of out */
    float* ws;               /* echr_decoder_row_grad_ws_floats(dec, ncols) floats */
} echr_row_grad_args;
int64_t echr_decoder_row_grad_ws_floats(const echr_dec_args* a, int32_t ncols);
int echr_decoder_row_grad(const echr_dec_args* a, const echr_dec_grads* g, const echr_row_grad_args* r, void* stream);
/* rows [Tv, Dc + Ht] = [c3d [Tv, Dc] | tap [Tv, Ht]] (the 'CC+CH' row source) */
int echr_clip_rows(const float* c3d, int32_t Dc, const float* tap, int32_t Ht, float* rows, int32_t Tv, void* stream);
/* Create the library's helper streams now (they are otherwise created by the first call that needs them) and submit one marker on each.
 * Call it once per process AFTER selecting the device and BEFORE anything else creates streams -- in particular before the RCCL communicator
 * is set up (torch.distributed.init_process_group with device_id): this runtime spreads streams over a handful of hardware queues in creation
 * order, and helper streams created behind RCCL's land on queues they share with each other -- the backward tail's three streams then
 * serialise (measured on one MI355X, single-rank communicator: 1.64 vs 1.49 ms per c3 iteration).  Returns 0, or -ENODEV without a device. */
int echr_streams_init(void);

int64_t echr_decoder_ws_floats(const echr_dec_args* a);
int64_t echr_decoder_ws_bwd_floats(const echr_dec_args* a);
int echr_decoder_fwd(const echr_dec_args* a, const echr_dropout* drop, void* stream);
/* The part of echr_decoder_fwd that does not read the event context (operand packs, P_all = ctx2att over the video rows, token
 * embedding, the token-side gate pre-activations of all S*N rows): started on a library-owned second stream, forked from `stream`, so
 * that it overlaps the event encoder (echr_event_pool_gather_fwd + echr_tsrm_fwd) the caller runs next on `stream`.  a->event may be
 * NULL here.  The following echr_decoder_fwd call must pass the same workspace with a->prepared = 1; it joins the streams. */
int echr_decoder_fwd_prepare(const echr_dec_args* a, void* stream);
/* Abandon a prepare whose echr_decoder_fwd will not follow (the caller changed its mind, or failed in between): `stream` waits for the
 * second stream, so the workspace may be released or reused in `stream` order afterwards.  A no-op when nothing is pending. */
int echr_decoder_fwd_prepare_cancel(void* stream);
int echr_decoder_bwd(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, void* stream);

/* ONE decoder timestep with the recurrent state passed in and out: OldModel.get_logprobs_state (models/OldModel_NEW.py:133-137) =
 * embed -> ThreeStream_Core.forward (:801-823, incl. Attention.forward :376-401) -> dropout -> logit -> log_softmax.
 * a: S is ignored (treated as 1), tokens = it [N] int32, logp = out [N,V1], ws from echr_decoder_ws_floats with S = 1.
 * h_in / c_in / h_out / c_out: [3,N,H] (the reference's `state` tuple; h holds the DROPPED outputs, :810,814,818,821).
 * drop->offset selects the dropout stream of this call (training mode).  Forward only; bitwise reproducible. */
int echr_decoder_step(const echr_dec_args* a, const float* h_in, const float* c_in, float* h_out, float* c_out,
                      const echr_dropout* drop, void* stream);

/* masked NLL of LanguageModelCriterion on log-probs [N,S,V1]: loss (device scalar) */
int echr_nll_loss_fwd(const float* logp, const int32_t* target, const float* mask, float* loss, int32_t N, int32_t S,
                      int32_t V1, void* stream);
/* the same on int64 targets (torch.LongTensor labels as train.py:298-303 passes them) */
int echr_nll_loss_fwd_i64(const float* logp, const int64_t* target, const float* mask, float* loss, int32_t N, int32_t S,
                          int32_t V1, void* stream);

/* backward of echr_nll_loss_fwd in one pass: g_logp [N,S,V1] (fully written); fwd_out = the 2-float output of the forward
 * (loss, sum(mask)), g_loss = upstream scalar gradient (device) */
int echr_nll_loss_bwd(const int32_t* target, const float* mask, const float* fwd_out, const float* g_loss, float* g_logp,
                      int32_t N, int32_t S, int32_t V1, void* stream);
int echr_nll_loss_bwd_i64(const int64_t* target, const float* mask, const float* fwd_out, const float* g_loss, float* g_logp,
                          int32_t N, int32_t S, int32_t V1, void* stream);

/* sampler (greedy or multinomial): runs seq_len+1 decoder steps on device without host syncs.
 * seq [N,seq_len] int64 (zero after a row finished), seq_logp [N,seq_len] fp32,
 * n_unfinished [seq_len+1] int32: number of unfinished rows after step t (the host trims the output
 * at the first t >= 1 with n_unfinished[t] == 0, as OldModel.sample's break does). */
typedef struct {
    echr_dec_args dec;       /* S, tokens, logp unused */
    int32_t seq_len;
    int64_t* seq;
    float* seq_logp;
    int32_t* n_unfinished;
    float* ws_sample;        /* echr_sampler_ws_floats */
    int32_t multinomial;     /* 0 = greedy arg-max (sample_max = 1, lowest index on ties); 1 = draw from softmax(logp / temperature)
                                (OldModel_NEW.py:160-168, sample_max = 0) with the library's Philox stream keyed by (seed, row, step):
                                reproducible per seed, the reference's distribution but not torch.multinomial's random stream */
    float temperature;       /* multinomial only; <= 0 means 1 */
    uint64_t seed;
    float* tables;           /* optional cache of the parameter-only operands of the persistent greedy decoder (token-side gate tables
                                embed . W_ih_k[:, :E]^T, logit-weight image): echr_sampler_table_floats floats, owned by the caller.  NULL:
                                they are rebuilt inside ws_sample on every call (~0.15 ms at V1 = 5001) */
    int32_t tables_valid;    /* 1: `tables` holds the operands of the CURRENT parameters (skip the rebuild); 0: rebuild into `tables` */
} echr_sample_args;
int64_t echr_sampler_ws_floats(const echr_dec_args* a);
int64_t echr_sampler_table_floats(const echr_dec_args* a);      /* 0 when the persistent decoder does not apply to these shapes / settings */
int echr_decoder_sample(const echr_sample_args* a, void* stream);
/* The sampled pass of self-critical training (CaptionGenerator.py:32-37 -> OldModel.sample with sample_max = 0 while the model is in
 * training mode, OldModel_NEW.py:139-187): the multinomial decode (a->multinomial must be 1) with the decoder's dropout ACTIVE, its masks
 * those of echr_decoder_fwd's step t under the same `drop` (keyed by element, step t, site, drop->offset), so a teacher-forced
 * echr_decoder_fwd on the tokens [0 | seq | 0] with the same `drop` reproduces seq_logp at every position up to a row's <eos>.  Always
 * the launch-per-step chain (the persistent decoder has neither draws nor dropout); its own ws / ws_sample, like echr_decoder_sample. */
int echr_decoder_sample_train(const echr_sample_args* a, const echr_dropout* drop, void* stream);

/* Beam search (OldModel.sample with opt beam_size = B, 1 <= B <= min(16, V1)): seq_len decision steps on device without host syncs,
 * eval mode, every event independently.  Per step: candidates s_j + logp_j[v] (fp32 log-softmax, no length penalty) over the event's
 * alive slots j and every token v; the B largest win, ties to the smaller j then the smaller v; new slot k is the k-th winner and
 * continues its parent's LSTM state.  A winner with v == 0 (<eos>), or any winner at the last step, finishes; the event's result is
 * replaced only by a finished hypothesis with a strictly greater score (slot order within a step).  B = 1 is the greedy decode up to
 * each row's first <eos>.  Bitwise reproducible. */
typedef struct {
    echr_dec_args dec;       /* N = events * beam_size rows, event-major (slot j of event n is row n*B + j): event, ev_start, ev_len and
                                h0 repeated B times per event; rows_disjoint 0; S, tokens, logp unused; ws from echr_decoder_ws_floats
                                with S = seq_len */
    int32_t beam_size;
    int32_t seq_len;
    int64_t* seq;            /* out [N/B, seq_len]: the result's words, then zeros */
    float* seq_logp;         /* out [N/B, seq_len]: its token log-probs, <eos> included (at position words[n] < seq_len), then zeros */
    float* score;            /* out [N/B]: the sum of its token log-probs, <eos> included */
    int32_t* words;          /* out [N/B + 1]: words per event (seq_len when it never emitted <eos>), then their maximum (the host's one
                                read: the output width) */
    float* ws_beam;          /* echr_beam_ws_floats */
} echr_beam_args;
int64_t echr_beam_ws_floats(const echr_beam_args* a);
int echr_decoder_beam(const echr_beam_args* a, void* stream);

/* Self-critical training on gathered log-probs (the module path; the one-call path is echr_train_step_rw).
 * echr_gather_tokens_fwd: out [N,T] = logp [N,S,V1] at (n, t, seq[n,t]), t < T <= S; _bwd writes g_logp [N,S,V1] in full (zero but there).
 * echr_reward_loss_fwd: RewardCriterion (misc/utils.py:48-59), mask[n,0] = 1, mask[n,t] = (seq[n,t-1] > 0):
 *   out[0] = sum(-input * reward * mask) / sum(mask) (no epsilon), out[1] = sum(mask); input / reward [N,T], seq int64 [N,T].
 * echr_reward_loss_bwd: g_input [N,T] = -reward * mask / fwd_out[1] * g_loss[0]. */
int echr_gather_tokens_fwd(const float* logp, const int64_t* seq, float* out, int32_t N, int32_t S, int32_t T, int32_t V1, void* stream);
int echr_gather_tokens_bwd(const float* g_out, const int64_t* seq, float* g_logp, int32_t N, int32_t S, int32_t T, int32_t V1, void* stream);
int echr_reward_loss_fwd(const float* input, const int64_t* seq, const float* reward, float* out, int32_t N, int32_t T, void* stream);
int echr_reward_loss_bwd(const int64_t* seq, const float* reward, const float* fwd_out, const float* g_loss, float* g_input,
                         int32_t N, int32_t T, void* stream);

/* CIDEr-D over token ids: the reward of self-critical training, score(sampled) - score(greedy), and a validation
 * metric without external tools.  The sequence of candidate row n under seq_length L is the l tokens before its first 0 among columns
 * < T (l = T when there is none), then one end token 0 iff l < L; columns >= T are never read.  References arrive in that form already.
 * For n = 1..4: w(g) = tf(g) * idf(g) over the order-n n-grams g, norm_n = sqrt(sum w^2); against reference r,
 *   val_n = sum_{g in h} min(w_h(g), w_r(g)) * w_r(g), divided by norm_n(h) * norm_n(r) iff both are non-zero, times
 *   exp(-(len_h - len_r)^2 / 72)  (sigma = 6; len counts the end token);   score = 10 * mean_n(sum_r val_n) / R.
 * idf comes from a table of exact keys -- key(g) = sum_i (tok_i + 1) << 16 i, i < n, tokens <= 65534 -- sorted strictly increasing as
 * uint64, with idf[k] = log(n_docs) - log(max(1, df[k])); an n-gram that is not in the table has idf_unseen = log(n_docs).
 * All arithmetic is fp64 in one fixed order, one workgroup per row: bitwise reproducible and independent of which rows share a launch.
 * out[n] = score, or weight * (score - base[n]) when `base` is given (the greedy scores of a previous call: the reward). */
typedef struct {
    int32_t N;                   /* candidate rows */
    int32_t L;                   /* the model's seq_length, 1 .. 63 */
    const void* cand;            /* [N, >= T] token ids, int64 (cand_i32 = 0) or int32 (1): element (n, t) at n * ld + t * cs */
    int32_t cand_i32;
    int32_t T;                   /* the width, 0 .. L; used when counts == NULL */
    int64_t ld, cs;              /* row and column stride of cand in elements */
    const int32_t* counts;       /* optional: a decode's n_unfinished [L + 1]; the width is t - 1 for the first t in 1 .. L with
                                    counts[t] == 0, else L (what the host cuts echr_decoder_sample's output at) */
    const int32_t* refs;         /* [R_tot, L] reference sequences, zero-padded */
    const int32_t* ref_len;      /* [R_tot] their lengths, 1 .. L, end token included */
    const int32_t* ref_offset;   /* [N + 1]: row n is scored against references ref_offset[n] .. ref_offset[n + 1] - 1 (at least one;
                                    a row without any scores 0) */
    int32_t R_tot;
    int32_t n_keys;              /* table entries, 0 = empty */
    const uint64_t* keys;        /* [n_keys] strictly increasing */
    const double* idf;           /* [n_keys] */
    double idf_unseen;
    const float* base;           /* optional [N] */
    float weight;                /* with base only */
    float* out;                  /* [N] */
} echr_ciderd_args;
int echr_ciderd_score(const echr_ciderd_args* a, void* stream);

/* Dense-caption scoring over token ids: the ANETcaptions protocol of the reference's
 * external_tool/densevid_eval/evaluate.py without METEOR -- tIoU matching at n_tau thresholds, Recall / Precision, and BLEU-1..4,
 * ROUGE-L and (optionally) CIDEr-D over the matched (prediction, ground truth) pairs.  Video v owns predictions
 * pred_offset[v] .. pred_offset[v + 1] - 1 (possibly none) and ground truths gt_offset[v] .. gt_offset[v + 1] - 1 (at least one).
 *   iou = max(0, min(e1, e2) - max(s1, s2)) / (min(max(e1, e2) - min(s1, s2), (e2 - s2) + (e1 - s1)) + 1e-8), fp64 in this order.
 * One struct serves the four entries; each reads the fields its stage names and validates them on the host before any launch.
 *  echr_densecap_match: count[k, i] = number of ground truths of prediction i's video with iou >= tau[k], 1 when there is none (the
 *    unmatched pair); pred_flag[k, i] = (any iou > tau[k]) | 2 * (no iou >= tau[k]); gt_hit[k, j] = any prediction of j's video with
 *    iou > tau[k].  No atomics: a thread owns a prediction or a ground truth.
 *  echr_densecap_fill: with start the exclusive scan of count (flattened [n_tau, N_tot], one entry more for the total), the pair list
 *    (pair_pred, pair_gt) ordered by threshold, video, prediction, ground truth; an unmatched pair has pair_gt = -1.
 *  echr_densecap_pair_stats: one wave per pair.  A caption's words are the tokens before its first 0 among its columns (< T for a
 *    candidate, < L for a reference row), all of them when there is none.  stats[p] = {match_1..4, len_c, len_r, lcs}: match_n the clipped
 *    count sum over the candidate's distinct order-n n-grams of min(tf_cand, tf_ref), lcs the longest common subsequence; an unmatched
 *    pair has zero matches, len_r = 1 and lcs 0.  rouge[p] = (1 + b^2) P R / (R + b^2 P), P = lcs / len_c, R = lcs / len_r, b = 1.2, 0
 *    unless both are positive.
 *  echr_densecap_reduce: video[k, v, :] = {recall, precision, Bleu_1..4, ROUGE_L, CIDErD, pairs, unmatched pairs} of video v at tau[k]
 *    (integer sums; BLEU in fp64 with p_n = (match_n + 1e-15) / (guess_n + 1e-9) and the brevity penalty of (c + 1e-15) / (r + 1e-9); the
 *    ROUGE-L and CIDEr-D means summed in pair order), and mean[k, :] the first eight averaged over the V videos in video order.  With
 *    stats == NULL (no captions) the language columns are 0.  Bitwise reproducible; a video's numbers do not depend on the others. */
#define ECHR_DENSECAP_MAX_TAU 8
#define ECHR_DENSECAP_VIDEO_COLS 10
#define ECHR_DENSECAP_MEAN_COLS 8
#define ECHR_DENSECAP_STATS 7
typedef struct {
    int32_t V, n_tau;            /* videos; thresholds, 1 .. ECHR_DENSECAP_MAX_TAU */
    int32_t N_tot, G_tot;        /* predictions and ground truths of the call */
    const double* pred_stamps;   /* [N_tot, 2] seconds */
    const int32_t* pred_offset;  /* [V + 1] */
    const double* gt_stamps;     /* [G_tot, 2] */
    const int32_t* gt_offset;    /* [V + 1] */
    const double* tau;           /* [n_tau], device memory */
    int32_t* count;              /* match out [n_tau, N_tot] */
    int32_t* pred_flag;          /* match out [n_tau, N_tot] */
    int32_t* gt_hit;             /* match out [n_tau, G_tot] */
    const int64_t* start;        /* [n_tau * N_tot + 1] exclusive scan of count */
    int64_t P_tot;               /* start's last entry: pairs over all thresholds, < 2^31 */
    int32_t* pair_pred;          /* fill out [P_tot] prediction row */
    int32_t* pair_gt;            /* fill out [P_tot] ground-truth row or -1 */
    int32_t L;                   /* seq_length, 1 .. 63: the width of refs */
    int32_t T;                   /* columns of cand, 0 .. 63 */
    const void* cand;            /* [N_tot, T] token ids, int64 (cand_i32 = 0) or int32 (1): element (n, t) at n * ld + t * cs */
    int32_t cand_i32;
    int64_t ld, cs;
    const int32_t* refs;         /* [G_tot, L] one reference per ground truth, zero-padded */
    int32_t* stats;              /* pair_stats out [P_tot, ECHR_DENSECAP_STATS] */
    double* rouge;               /* pair_stats out [P_tot] */
    const float* cider;          /* optional [P_tot]: the pairs' CIDEr-D (0 at unmatched pairs) */
    double* video;               /* reduce out [n_tau, V, ECHR_DENSECAP_VIDEO_COLS] */
    double* mean;                /* reduce out [n_tau, ECHR_DENSECAP_MEAN_COLS] */
} echr_densecap_args;
int echr_densecap_match(const echr_densecap_args* a, void* stream);
int echr_densecap_fill(const echr_densecap_args* a, void* stream);
int echr_densecap_pair_stats(const echr_densecap_args* a, void* stream);
int echr_densecap_reduce(const echr_densecap_args* a, void* stream);

/* Proposal targets and caption-event samples from ground-truth segments: what dataloader.get_vid_data / get_data /
 * get_shuffle_list build per video on the host (dataloader.py:266-281, 339-357, 107-109, 124, 615-639), over a multi-video batch in the
 * concatenated [T_tot, K] layout.  Video v owns rows row_offset[v] .. row_offset[v + 1] - 1 (at least one) and the ground-truth featstamps
 * gt[gt_offset[v] .. gt_offset[v + 1] - 1] = (start, end), local to the video, possibly none, at most ECHR_TARGETS_MAX_GT.  All vectors are
 * device memory; that the offsets grow and that 0 <= start < end <= T_v - 1 is the caller's contract (echr_amd.targets checks its host
 * copies) -- offsets outside the buffers select nothing and no access leaves the buffers.  G_max is the caller's statement of the largest
 * per-video segment count: what the library can refuse before the launch.
 *  echr_tap_targets_batch, for local row t and column k:
 *    valid = t >= k + 1;  tap_masks = valid;  iou = 0 and gts_index = 0 where not valid.  Where valid the anchor is [a, t], a = t - k - 1, and
 *    for each ground truth i in order, with s = start - 0.01, e = end + 0.01:
 *      inter = max(0, min(e, t) - max(s, a));  uni = min(max(e, t) - min(s, a), ((e - s) + t) - a);  ov = inter / (uni + 1e-8)
 *    in fp64 in this order; the running maximum is replaced when ov >= best, from best = 0.0, index = -1: ties go to the later ground truth,
 *    an anchor that overlaps nothing gets G_v - 1, a video without segments -1.  iou = (float)best;  tap_labels = iou >= (float)iou_threshold;
 *    good = iou >= (float)iou_threshold_good (fp32 compares);  good_gt = gts_index where good, else -1;  n_good[v] = the number of good cells.
 *    Both thresholds must be positive.  Every operation is a correctly rounded fp64 add, subtract, compare or divide, with no product: the
 *    outputs equal the host's bit for bit.
 *  echr_prop_events_batch: events[v, i, :] = (t, k, gt) of video v's i-th listed proposal, -1 behind the list; cap = prop_sample_num.
 *    sampled = 0: every good cell in row-major (t, k) order, cut at cap; n_events[v] = the uncut count (`*_select_list_eval`).
 *    sampled = 1: cell p = t * K + k draws word p & 3 of Philox-4x32-10 with counter (p >> 2, draw[v], 7, 0) and key (seed lo, seed hi) -- site 7
 *    of echr_amd/philox.py; the min(n_good, cap) cells with the smallest (word, p) are listed in ascending (word, p) order: a uniform subset
 *    in uniform order up to ties of words, which position breaks; n_events[v] = the listed count.  A video's list depends on its own cells,
 *    seed and draw[v] alone.  Bitwise reproducible. */
#define ECHR_TARGETS_MAX_GT 1024
#define ECHR_TARGETS_MAX_VIDEOS 65535
#define ECHR_TARGETS_MAX_K 65536
#define ECHR_PROP_MAX_SAMPLE 1024
int echr_tap_targets_batch(const int32_t* row_offset, const int32_t* gt_offset, const int32_t* gt, int32_t V, int32_t T_tot, int32_t G_tot,
                           int32_t G_max, int32_t K, double iou_threshold, double iou_threshold_good, float* iou, int32_t* gts_index,
                           float* tap_masks, float* tap_labels, int32_t* good_gt, int32_t* n_good, void* stream);
int echr_prop_events_batch(const int32_t* good_gt, const int32_t* row_offset, int32_t V, int32_t T_tot, int32_t K, int32_t cap, int32_t sampled,
                           uint64_t seed, const int32_t* draw, int32_t* events, int32_t* n_events, void* stream);

/* Captioning external temporal-event proposals (the reference's flag_eval_what = 'SOTA_TEP') over a multi-video batch.
 * Video v owns the proposals prop_offset[v] .. prop_offset[v + 1] - 1 (possibly none, at most ECHR_EXTPROPS_MAX_P) of stamps [P_tot, 2]
 * (start, end in seconds) and prop_scores [P_tot], both fp64.  All vectors are device memory; that the offsets grow, that every value is
 * finite and that end >= start is the caller's contract (echr_amd.extprops checks its host copies) -- offsets outside the buffers select
 * nothing and no access leaves the buffers.  P_max is the caller's statement of the largest per-video count: what the library can refuse
 * before the launch.
 *  echr_nms_segments_batch: eval_utils.gettopN_nms (eval_utils.py:230-256) per video, a workgroup each.  area_i = (t2_i - t1_i) + 1e-3; the
 *    alive set starts as everything; a round takes the alive proposal i with the largest prop_score (ties: the largest index -- the last
 *    element of a stable ascending sort) and forms for every alive j, i included,
 *      wh = max(0, (min(t2_i, t2_j) - max(t1_i, t1_j)) + 1e-3);  o = wh / ((area_i + area_j) - wh)
 *    in fp64 in this order (no product: the comparison bits are numpy's).  The cluster is the alive j with o >= nms_overlap; the round's pick
 *    is its member with the largest sent_score (null: prop_scores), ties to the member that comes first in ascending (prop_score, index)
 *    order; alive becomes the alive j with o <= nms_overlap -- a proposal whose o equals the threshold is clustered AND stays alive, as in
 *    the reference.  Rounds end when nothing is alive or `rounds` picks are made.  pick[v, 0 .. count[v] - 1] (row stride `rounds`) are the
 *    picks in round order, video-local indices, duplicates as they occur, -1 behind the list.  0 <= nms_overlap < 1: at 1 the best never
 *    leaves the alive set.
 *  echr_ext_proposals_batch: the selection of eval_utils.py:88-104, then dataloader.timestamp_to_featstamp and the crop of
 *    dataloader.py:515-520.  A video's proposals are walked in file order; i is kept if it occurs in pick[v, 0 .. pick_count[v] - 1] (pick
 *    null: every proposal is picked, the nms_threshold <= 0 branch) and prop_scores[i] >= val_score_thres (fp64); the walk ends after topN
 *    kept.  Per kept proposal, with T = rows[v] (a video with T < 2 selects nothing) and duration[v] > 0, in fp64:
 *      s = clamp(round((start / duration) * T), 0, T - 2);  e = clamp(round((end / duration) * T), s + 1, T - 1)      (round: half away from zero)
 *    and, with crop = 1, where e - s >= K + 1:  r = (w * (e - s - K + 1)) >> 32,  s = s + r,  e = s + K,  w = word i & 3 of Philox-4x32-10
 *    with counter (i >> 2, draw[v], 8, 0) and key (seed lo, seed hi) -- site 8 of echr_amd/philox.py.  A video's list depends on its own
 *    proposals, seed and draw[v] alone.  Outputs, compacted over the batch in video order: index (the kept video-local i, ascending per
 *    video), ind = e, soi = (s, e + 1), each of capacity `cap` entries (at least the sum of min(P_v, topN)); count[v] and event_offset[v],
 *    with the total in count[V] and event_offset[V].  stage is a scratch of 3 * P_tot int32. */
#define ECHR_EXTPROPS_MAX_P 4096
#define ECHR_EXTPROPS_MAX_VIDEOS 65535
int echr_nms_segments_batch(const double* stamps, const double* prop_scores, const double* sent_score, const int32_t* prop_offset, int32_t V,
                            int32_t P_tot, int32_t P_max, double nms_overlap, int32_t rounds, int32_t* pick, int32_t* count, void* stream);
int echr_ext_proposals_batch(const double* stamps, const double* prop_scores, const int32_t* prop_offset, const int32_t* rows,
                             const double* duration, const int32_t* pick, const int32_t* pick_count, int32_t rounds, int32_t V, int32_t P_tot,
                             int32_t P_max, int32_t K, int32_t topN, double val_score_thres, int32_t crop, uint64_t seed, const int32_t* draw,
                             int32_t* stage, int32_t cap, int32_t* count, int32_t* event_offset, int32_t* index, int32_t* ind, int32_t* soi,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * SST proposal encoder.  Replaces models/sst_model.py:31-40 (nn.LSTM over one video + Linear + sigmoid)
 * and TAPModelCriterion (misc/utils.py:78-99).  Parameters use nn.LSTM's layout: w_ih[l] [4H, D or H], w_hh[l] [4H,H],
 * gate order i,f,g,o.  p_drop = inter-layer dropout (applied to layer 0's output while training; site 5 of echr_dropout).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t T, D, H, K;
    float p_drop;
    const float* w_ih[2];
    const float* w_hh[2];
    const float* b_ih[2];
    const float* b_hh[2];
    const float *w_sc, *b_sc;       /* scores Linear [K,H],[K] */
    const float* x;                 /* [T,D] C3D features of one video */
    float* ws;                      /* saved activations, echr_sst_ws_floats */
    float* tap_feats;               /* out [T,H]: top-layer hidden states */
    float* scores;                  /* out [T,K]: sigmoid proposal scores */
} echr_sst_args;

typedef struct {
    float* g_w_ih[2];
    float* g_w_hh[2];
    float* g_b_ih[2];
    float* g_b_hh[2];
    float *g_w_sc, *g_b_sc;
    const float* g_tap;             /* [T,H] or NULL */
    const float* g_scores;          /* [T,K] or NULL */
    float* ws_bwd;                  /* scratch, echr_sst_ws_bwd_floats */
    int32_t zeroed;                 /* 1: every parameter-gradient buffer arrives zero-filled (flat arena, one fill by the caller): the library
                                       accumulates into them instead of zero-filling each split-K product's output itself */
} echr_sst_grads;

int64_t echr_sst_ws_floats(int32_t T, int32_t D, int32_t H, int32_t K);
int64_t echr_sst_ws_bwd_floats(int32_t T, int32_t D, int32_t H, int32_t K);
int echr_sst_fwd(const echr_sst_args* a, const echr_dropout* drop, void* stream);
/* The two halves of echr_sst_fwd as calls of their own (round 6): the recurrence -> tap_feats (models/sst_model.py:33-37), and the proposal head
 * scores = sigmoid(tap_feats . W_sc^T + b_sc) (:38-39) from the tap_feats of the same arguments.  The joint iteration's caption side waits for
 * tap_feats alone; its caller queues the head behind the caption call (fused.JointTrainStep). */
int echr_sst_fwd_states(const echr_sst_args* a, const echr_dropout* drop, void* stream);
int echr_sst_head_fwd(const echr_sst_args* a, void* stream);
int echr_sst_bwd(const echr_sst_args* a, const echr_sst_grads* g, const echr_dropout* drop, void* stream);
/* The proposal encoder over a multi-video batch (the producer of a batch's tap_feats; stage 1 of the reference's recipe sums the gradients
 * of m_batch videos, train.py:281-283,313-317).  a->T is T_tot; x, tap_feats, scores and every saved activation use the concatenated
 * [T_tot, .] layout of the caption path's batches: video v owns rows [row_offset[v], row_offset[v+1]).  Every video starts from the zero
 * state.  The rows of video v equal what echr_sst_fwd gives for that video alone; parameter gradients are the SUM over the videos.  One
 * dropout counter per call: the inter-layer mask is keyed by the batch-global element (row_offset[v] + t) * H + u at site 5.  These entries
 * and the single-video ones above are wrappers around one forward and one backward: a batch of ONE video is echr_sst_fwd / echr_sst_bwd
 * -- the same launches, the same bits, the device row_offset is not read, and a refusal behind the argument checks names "sst_fwd" /
 * "sst_bwd".  Products over rows run once over T_tot rows; the recurrences carry a video axis: the persistent form (H = 512) runs up to
 * echr_sst_batch_group() videos through the register-resident weight slices per launch and splits a larger batch into ceil(V / group)
 * launches, the launch-per-step wavefront (any H) puts the videos on the grid.  Gradient buffers, `zeroed` and the deterministic switch
 * behave as in echr_sst_bwd. */
typedef struct {
    int32_t n_videos;                   /* V >= 1 */
    const int32_t* row_offset;          /* device [V+1], row_offset[0] = 0, strictly increasing, row_offset[V] = a->T */
    const int32_t* row_offset_host;     /* the same values in host memory (the library sizes its loops and groups from them) */
} echr_sst_batch;
int64_t echr_sst_batch_ws_floats(int32_t T_tot, int32_t D, int32_t H, int32_t K, int32_t V);
int64_t echr_sst_batch_ws_bwd_floats(int32_t T_tot, int32_t D, int32_t H, int32_t K, int32_t V);
int echr_sst_fwd_batch(const echr_sst_args* a, const echr_sst_batch* x, const echr_dropout* drop, void* stream);
int echr_sst_bwd_batch(const echr_sst_args* a, const echr_sst_batch* x, const echr_sst_grads* g, const echr_dropout* drop, void* stream);
int echr_sst_batch_group(void);         /* videos one persistent launch carries; a larger V is split by the library */
/* weighted BCE of the proposal head: loss (device scalar) and its gradient w.r.t. the scores */
int echr_tap_bce_fwd(const float* scores, const float* masks, const float* labels, const float* w1, float* loss, int32_t T,
                     int32_t K, void* stream);
/* the same loss with a caller-provided scratch of 64 floats (`partials`): 64 workgroups + a final fixed-order add instead of one workgroup
 * (bit-reproducible either way; what echr_amd uses) */
int echr_tap_bce_fwd_ws(const float* scores, const float* masks, const float* labels, const float* w1, float* loss, float* partials,
                        int32_t T, int32_t K, void* stream);
int echr_tap_bce_bwd(const float* scores, const float* masks, const float* labels, const float* w1, const float* g_loss,
                     float* g_scores, int32_t T, int32_t K, void* stream);
/* The criterion over a multi-video batch: scores / masks / labels are the concatenated [T_tot, K] matrices, row_offset device int32 [V+1].
 * video_loss[v] = TAPModelCriterion of video v (its own mean over T_v x K, times K), loss_sum (optional) = their sum in video order, no 1/V.
 * w1_ld = 0: one [K] weight vector for all videos; w1_ld = K: w1 is [V, K].  partials: scratch of 64 * V floats.  Every sum runs in one
 * fixed order; video 0 of a one-video batch equals echr_tap_bce_fwd_ws bit for bit.
 * bwd: g_scores[t, k] = g_loss * w * d * m / T_v for the video v that owns row t (one launch over T_tot * K; row_offset[V] must be T_tot).
 * Precondition (the offsets live on the device, the entries cannot check it): row_offset[0] = 0 and row_offset grows STRICTLY -- every video
 * owns at least one row.  A video without rows would make its mean 0 / 0 and the gradient divide by T_v = 0. */
int echr_tap_bce_fwd_batch(const float* scores, const float* masks, const float* labels, const float* w1, int32_t w1_ld,
                           const int32_t* row_offset, int32_t V, int32_t K, float* video_loss, float* loss_sum, float* partials, void* stream);
int echr_tap_bce_bwd_batch(const float* scores, const float* masks, const float* labels, const float* w1, int32_t w1_ld,
                           const int32_t* row_offset, int32_t V, int32_t K, int32_t T_tot, const float* g_loss, float* g_scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Proposal selection: the index outputs of eval_utils.gettop1000 (eval_utils.py:259-287), bit-exact.
 * Output buffers must hold T*K entries (ties at the threshold are all kept); out_count[0] = number written.
 * ---------------------------------------------------------------------------------------------- */
int echr_top_proposals(const float* scores, const float* mask, int32_t T, int32_t K, int32_t topN, float val_thres,
                       int32_t* out_ind, int32_t* out_feat, float* out_conf, int32_t* out_count, void* stream);

/* Greedy temporal NMS variant (eval_utils.gettop1000_nms, eval_utils.py:290-331): candidates (n, k < min(n,K)) = [n-k, n+1], picked by
 * descending score until topN, suppressing inclusive-IoU > overlap (float64, the reference's operation order).  Equal scores: the
 * later candidate wins (the reference's unstable argsort leaves ties undefined).  scratch: T*K floats.  out_feat [topN,2], out_conf
 * [topN] in pick order; out_count[0] = number of picks. */
int echr_top_proposals_nms(const float* scores, int32_t T, int32_t K, int32_t topN, double overlap, float* scratch,
                           int32_t* out_feat, float* out_conf, int32_t* out_count, void* stream);

/* Both selections over the V videos of a batch in ONE call: scores [T_tot, K] is the concatenated output of echr_sst_fwd_batch,
 * row_offset int32 [V+1] (device) names video v's rows, workgroup v runs the single-video algorithm over them with n and k local to the
 * video; a second one-workgroup launch scans the counts and closes the gaps between the videos' lists.  No host synchronisation.
 *   mask [T_tot, K] or NULL (threshold entry): NULL = the causal mask n_local >= k.
 *   count int32 [V+2]: picks per video, their total, the largest interval length max(e - s) over all picks (0 without a pick).
 *   event_offset int32 [V+1]: exclusive scan of the counts.   vid int32 [N_tot]: video of every pick.
 *   ind [N_tot], feat [N_tot,2]: video-local anchors / intervals, videos in order, inside a video the single-video order;
 *   ind_abs, feat_abs: the same + row_offset[vid] (rows of the concatenated matrices);   conf [N_tot].
 * Capacity of vid / ind / feat / ind_abs / feat_abs / conf in entries: T_tot*K (threshold: ties can exceed topN), V*topN (NMS).
 * live (NMS): T_tot*K floats of scratch.  A video whose offsets are not 0 <= row_offset[v] < row_offset[v+1] <= T_tot selects nothing. */
int echr_top_proposals_batch(const float* scores, const float* mask, const int32_t* row_offset, int32_t T_tot, int32_t V, int32_t K,
                             int32_t topN, float val_thres, int32_t* count, int32_t* event_offset, int32_t* vid, int32_t* ind,
                             int32_t* feat, int32_t* ind_abs, int32_t* feat_abs, float* conf, void* stream);
int echr_top_proposals_nms_batch(const float* scores, const int32_t* row_offset, int32_t T_tot, int32_t V, int32_t K, int32_t topN,
                                 double overlap, float* live, int32_t* count, int32_t* event_offset, int32_t* vid, int32_t* ind,
                                 int32_t* feat, int32_t* ind_abs, int32_t* feat_abs, float* conf, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused element-wise clamp(+-clip) + Adam (betas, eps, no weight decay, no amsgrad) over a flat
 * buffer.  Replaces misc/utils.py:107-111 + torch.optim.Adam.step as wired at train.py:209,315-317.
 * `step` is the 1-based step count; lr/betas/eps are doubles because torch derives 1-beta and the bias corrections
 * from the Python doubles (1 - 0.999f != 0.001).
 * ---------------------------------------------------------------------------------------------- */
int echr_clamp_adam(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1,
                    double beta2, double eps, float clip, void* stream);
/* The same, counting itself: `applied` (optional device word, one per optimiser state, zeroed by its owner) is incremented by the launch
 * iff the update was applied, i.e. not skipped under an unacknowledged asynchronous failure (see echr_check_async).  After a -62 the owner
 * reads the word (everything queued has retired by then) and sets its step count to the number of updates that really happened. */
int echr_clamp_adam_counted(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1,
                            double beta2, double eps, float clip, uint32_t* applied, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One training iteration of the caption path as ONE call.  Replaces the per-iteration protocol of train.py:281-317 around the hot
 * path -- zero_grad; cg_model(tap_feats, c3d_feats, lda_feats, labels, ind, soi, 'train') (CaptionGenerator.py:17-30);
 * LanguageModelCriterion (misc/utils.py:66-75); backward; clip_gradient; optimizer.step() -- for m_batch = 1 with the caption
 * model's parameters and gradients in flat buffers.  The entry sequences the library's own pieces (event pooling, TSRM encoder,
 * decoder forward / backward with the fused criterion gradient, clamp + Adam) on `stream`; the host pays one call instead of ~75.
 *
 * The caller fills: the parameter pointers and shapes of `tsrm` / `dec` (N, A, Tv, S, rows_disjoint included), dec.c3d, dec.video,
 * the gradient pointers of `tsrm_g` / `dec_g` (views of flat_g; dec_g.g_video optional), `drop`, and the fields below.  Every
 * other pointer of the four embedded structs (index vectors, event context, tokens, workspaces, log-probs, upstream gradients) is
 * set by the library from `ws`.
 * ---------------------------------------------------------------------------------------------- */
/* hand-over callback (echr_train_step_args.handover_cb); which = ECHR_HANDOVER_LOGIT or ECHR_HANDOVER_LSTM */
typedef void (*echr_handover_fn)(int32_t which, void* stream, void* user);
/* mid-call hook of the joint form (echr_train_step_args.mid_cb) */
typedef void (*echr_mid_fn)(void* stream, void* user);
typedef struct {
    echr_tsrm_args tsrm;
    echr_tsrm_grads tsrm_g;
    echr_dec_args dec;
    echr_dec_grads dec_g;
    echr_dropout drop;
    const float* tap;              /* [Tv,Ht] proposal-encoder states (tap_feats) */
    int32_t Ht;
    float* g_tap;                  /* optional [Tv,Ht], zero-filled by the caller: receives d loss / d tap_feats (joint training); NULL = tap is data */
    const int32_t* host_index;     /* HOST memory (any kind; copied into a pinned ring inside the call):
                                      ev_start[N] | ev_len[N] | ind[N] | tokens[S*N] (time-major input tokens, labels[:, t])
                                      | active[n_active] (below) | and, with host_nll = 1, targets int32 [N*S] | mask fp32 [N*S] */
    const void* nll_target;        /* device [N,S] targets (labels[:, 1:1+S]), int64 or int32 */
    int32_t nll_target_i64;
    const float* nll_mask;         /* device [N,S] */
    const float* g_loss;           /* device scalar: d objective / d loss (1 for plain training) */
    float* loss;                   /* device [2]: out = (loss, sum(mask)) */
    float* ws;                     /* workspace, echr_train_step_ws_floats floats, 256-byte aligned */
    int64_t ws_floats;
    float* flat_g;                 /* the gradient arena (n_flat floats): zero-filled by the call, then accumulated into */
    int64_t n_flat;
    float *flat_p, *adam_m, *adam_v; /* parameter arena and Adam moments (do_step = 1) */
    int32_t adam_step;             /* 1-based step count of THIS update */
    double lr, beta1, beta2, eps;
    float clip;                    /* clip_gradient value (inf = none) */
    int32_t do_step;               /* 0: stop after the backward pass (the caller reduces / inspects flat_g and steps itself) */
    int32_t overlap_encoder;       /* 1: the decoder forward's event-independent part runs on the library's second stream beside the event encoder */
    int32_t forward_only;          /* 1: stop after the criterion (validation loss, eval_utils.py:148-152) */
    int32_t n_active;              /* > 0: host_index carries the n_active time-major rows t*N + n with a non-zero criterion mask (ascending);
                                      training then forms logits, d logits and the logit-layer products on those rows only (the masked-out
                                      label positions behind a caption's end -- half of all rows at S = 20 -- cannot reach the loss).  0: all rows */
    int32_t host_nll;              /* 1: targets and mask travel in host_index too (nll_target / nll_mask are ignored) */
    int32_t prepared;              /* 1: echr_train_step_prepare already ran with these arguments (see there) */
    int32_t defer_update;          /* 1 (with g_tap and do_step): joint 'tap_cg' iteration -- the call returns as soon as g_tap and the loss are
                                      final in `stream` order; the parameter gradients and the clamp + Adam update complete on library-owned
                                      streams beside whatever the caller queues next (the proposal encoder's backward, train.py:313).  The
                                      caller MUST call echr_stream_join(stream) before reading parameters or gradients or freeing ws;
                                      the next echr_train_step joins by itself */
    int32_t handover;              /* 1 (with do_step = 0): data-parallel hand-over points.  The backward pass records an event where the
                                      logit layer's gradients (g_w_logit, g_b_logit) become final and one where the three LSTM layers'
                                      gradients (g_w_ih / g_w_hh / g_b_ih / g_b_hh) do -- both long before the call's last kernel -- so the
                                      caller can start the collectives on those ranges of flat_g while the rest of the backward tail runs:
                                      echr_handover_wait(which, s) makes stream s wait for the point (train.py:281-283,313-317: the reference
                                      sums m_batch gradients before one clamp + step; the data-parallel form sums over ranks) */
    echr_handover_fn handover_cb;  /* optional (with handover = 1): called on the HOST, from inside the call, at each hand-over point -- right
                                      after the last launch that writes the range has been queued on `stream` (a library-owned stream).  What the
                                      callback queues on `stream`, or orders behind it, runs as soon as the range is final and beside the rest of
                                      the backward tail: a collective library that orders its own stream behind the caller's CURRENT stream needs
                                      no further stream or event (RCCL through torch.distributed: make `stream` current for the call).  The
                                      callback must not call back into this library and must not block on the device */
    void* handover_user;           /* passed through to handover_cb */
    uint32_t* adam_applied;        /* optional (do_step = 1): the optimiser state's count of applied updates, see echr_clamp_adam_counted */
    /* ---- the reference's non-recipe options on the one-call path (round 6; all zero / NULL = the ECHR recipe) ---- */
    int32_t event_parts;           /* event_context_type (CaptionGenerator.py:106-130): 0 or 3 = 'ER3' (pooled C3D rows | anchor state), 1 = 'ER1'
                                      (pooled rows only: tsrm.Din = dec.D), 2 = 'ER2' (anchor states only: tsrm.Din = Ht) */
    const float *w_init, *b_init;  /* CG_init_feats_type (OldModel_NEW.py:72-96): init_linear.weight [3H, Dtot] / .bias [3H]; h(-1) = c(-1) =
                                      init_linear(cat([video | event | clip.mean(1)])) with the parts init_use_* select.  NULL = zero state.
                                      (The persistent recurrence kernels start from zero: such a call runs the launch-per-phase recurrences.) */
    float *g_w_init, *g_b_init;    /* their gradient slots in flat_g */
    int32_t init_use_v, init_use_e, init_use_c;
    int32_t vh_offset;             /* 'VH' in video_context_type with g_tap: dec.video[vh_offset : vh_offset + Ht] is tap.mean(0) over tap_rows rows
                                      (formed by the caller, CaptionGenerator.py:95-99); d loss / d video of that span -- from the decoder and from
                                      init_linear -- is spread back over the rows of g_tap.  With it the call does not defer its update.  -1 or
                                      g_tap = NULL: the scene vector is data */
    int32_t tap_rows;              /* rows of tap / g_tap (only read with vh_offset >= 0) */
    echr_mid_fn mid_cb;            /* optional, joint form (defer_update = 1): called on the HOST from inside the call once everything that leads to
                                      g_tap and the loss has been queued on `stream`, BEFORE the parameter-gradient tail and the update are forked onto
                                      the library's streams.  What the callback queues on `stream` -- the proposal encoder's backward and update,
                                      train.py:313 -- starts right behind g_tap, and the tail is ordered BEHIND it (the proposal encoder's reverse
                                      recurrence is a 64-workgroup latency chain that loses more beside chip-filling kernels than the overlap
                                      gains).  Called exactly once per call that takes the deferred form, never otherwise; may call other entry
                                      points of this library on `stream`; must not block on the device */
    void* mid_user;
    int32_t event_direct;          /* event_context_type 'EC' / 'EH' (CaptionGenerator.py:106-137): the event vector without the event encoder.
                                      0 = through the encoder (event_parts; everything above).  1 = 'EC': the mean of the event's C3D rows
                                      (dec.De = the C3D width), 2 = 'EH': the proposal encoder's state at the event's anchor, tap[ind]
                                      (dec.De = Ht; tap must be given).  echr_event_pool_gather_fwd writes the [N, De] vectors straight into the
                                      decoder's event input; tsrm / tsrm_g / event_parts are not read, the workspace has no encoder regions, no
                                      position branch is forked.  Backward: the decoder's d event (plus init_linear's with init_use_e) goes,
                                      with g_tap and value 2, to echr_event_pool_gather_bwd(g_event, ind, g_tap, N, 0, Ht); with value 1 it
                                      reaches nothing.  defer_update is ignored (the plain form runs, mid_cb is not called); prepared = 1 is
                                      refused -- echr_train_step_prepare's work ahead of tap_feats is the decoder's event-independent part
                                      plus the encoder's position branch, and the callers of a direct context run without it.  Everything else
                                      (hand-over points, stage-ahead, n_active, host_nll, weights, per-video losses, 'VH', clip rows) is unchanged */
} echr_train_step_args;
int64_t echr_train_step_ws_floats(const echr_train_step_args* a);
/* Back-to-back calls (round 6, "stage-ahead"): a call that ends with its own update (do_step = 1, not deferred) lets the NEXT call on the same
 * stream, workspace and arena start its index staging copy and the event encoder's position embedding -- which read host_index and nothing the
 * update writes -- on a library stream beside that update; everything else of the next call is ordered behind the update as before.  Nothing
 * changes for the caller: host_index is copied inside the call, and `ws` must stay untouched between calls as it always had to (it holds the
 * saved activations until the call's last kernel).  ECHR_STAGE_AHEAD=0 in the environment switches it off. */
int echr_train_step(const echr_train_step_args* a, void* stream);
/* Self-critical training step (RewardCriterion, misc/utils.py:48-59): echr_train_step with the criterion
 *   loss = sum(-logp[target] * w) / sum(mask),   w[n,t] = reward[n,t] * mask[n,t]   (signed; no epsilon in the denominator)
 * for the teacher-forced tokens [0 | gen_result | 0].  Rows with a non-zero mask are the active rows, whatever their reward.
 * `weight`: device [N,S] fp32 with host_nll = 0; with host_nll = 1 host_index carries it behind the mask (| weights fp32 [N*S]) and
 * `weight` must be NULL (both at once is an error).
 * Workspace: echr_train_step_rw_ws_floats (the index region holds the weights too).  prepared must be 0.  Every other field, the
 * applied-update counting and stage-ahead behave as in echr_train_step: the sampled / greedy decodes a caller runs between two calls use
 * workspaces of their own and are ordered on the caller's stream, so they need no extra guard. */
int64_t echr_train_step_rw_ws_floats(const echr_train_step_args* a);
int echr_train_step_rw(const echr_train_step_args* a, const float* weight, void* stream);
/* Optional first half for the joint 'tap_cg' iteration (train.py:300-313): stages the index vectors and starts everything of the call that
 * does not read tap_feats (the decoder's event-independent part, the gradient-arena fill) on the library's prepare stream, so that it runs
 * beside the proposal encoder's forward the caller queues next.  Takes the arguments of the following echr_train_step (tap, g_tap, loss
 * slots may still be unset), which must then pass prepared = 1 and the same workspace.  Needs overlap_encoder = 1. */
int echr_train_step_prepare(const echr_train_step_args* a, void* stream);
/* echr_train_step (or, with rw = 1, echr_train_step_rw) with the frame-level context 'CH' or 'CC+CH'.  In `a`, dec.D / dec.Tv describe the
 * ROW SOURCE (D = Ht or Dc + Ht; Tv <= the rows of c3d and of tap) and dec.c3d is ignored: the library takes tap itself ('CH') or forms
 * [c3d | tap] in its workspace ('CC+CH').  The event encoder pools `c3d` [>= Tv, Dc].  With g_tap the clip-row gradient (echr_decoder_row_grad)
 * is added to g_tap and is final when the call returns; defer_update is then ignored (the plain form runs: the row gradient needs the
 * backward's attention stage, which the deferred form leaves on the helper streams).  Not with prepared = 1 nor with an initial state that
 * reads the clip (init_use_c). */
typedef struct {
    int32_t clip_parts;      /* 2 = 'CH', 3 = 'CC+CH' */
    int32_t Dc;              /* C3D width (video_dim) */
    const float* c3d;        /* [>= dec.Tv, Dc] C3D features */
    int32_t rw;              /* 1: reward-weighted criterion (echr_train_step_rw semantics) */
    const float* weight;     /* rw = 1 with host_nll = 0: device [N,S] weights; NULL otherwise */
} echr_clip_step_args;
int64_t echr_train_step_clip_ws_floats(const echr_train_step_args* a, const echr_clip_step_args* x);
int echr_train_step_clip(const echr_train_step_args* a, const echr_clip_step_args* x, void* stream);
/* ------------------------------------------------------------------------------------------------
 * Multi-video batches.  The entry points above take the events of ONE video (the reference's batch_size = 1, opts.py:187); the ones below
 * take the events of V >= 1 videos in one call.  The feature rows of the videos are concatenated ([sum T_v, D]); ev_start / ind are
 * batch-absolute row indices; events of a video are contiguous and videos keep their order (vid non-decreasing).  With equal dropout
 * masks a batched call equals V single-video calls:
 *   - scene context: one vector per video, `video` [V, Dv]; event n reads row vid[n] (echr_dec_args.video is ignored);
 *   - event encoder: an event attends to the events of its own video only (block-diagonal softmax; the position embedding is
 *     unchanged by a row offset);
 *   - criterion (echr_train_step_batch): loss = sum over v of LanguageModelCriterion of video v, each with its own normaliser
 *     sum(mask_v) + 1e-6 -- the caller passes the per-position weight w[n,t] = mask[n,t] / (sum(mask of video vid[n]) + 1e-6) and the
 *     library applies it with denominator 1; gradients are the SUM over the videos (train.py:281-283,313-317 with m_batch = V), then one
 *     clamp + Adam;
 *   - dropout: one forward-call counter per batched call, every site keyed by the batch-global element index;
 *   - decoding (echr_decoder_sample_batch greedy, echr_decoder_beam_batch beam search): every event decodes as it does alone; a
 *     single-video decode stops at the width of ITS longest caption, so the beam entry also reports that width per video.
 * Every entry takes the arguments of its single-video sibling plus this extension; the sibling's structs are unchanged.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_videos;            /* V */
    const int32_t* vid;          /* device [N]: video of event n, non-decreasing (echr_train_step_batch: may be NULL, see there) */
    const float* video;          /* device [V, Dv] scene vectors (the event encoder's entries do not read it) */
    float* g_video;              /* optional [V, Dv] out: d loss / d video (echr_dec_grads.g_video is ignored) */
    float* ws;                   /* decoder entries: scratch of echr_batch_ws_floats floats (per-event scene part of stream 2's gates, its per-video
                                    form and the per-video gate-gradient sums); only read and written inside the call.  echr_train_step_batch
                                    carves it from its own workspace and ignores this field */
} echr_batch_ext;
int64_t echr_batch_ws_floats(int32_t N, int32_t n_videos, int32_t H);
/* Scene contexts 'VC' / 'VH' of a batch: out[v*ld_out + c] = mean of x[r, c] over the rows r of segment v = [row_offset[v], row_offset[v+1])
 * (one launch for all n_seg segments; an empty segment is an error of the caller: its mean is written as 0);
 * bwd: gx[r, c] += g[v*ld_g + c] / rows(v) for the rows of segment v. */
int echr_seg_col_mean_fwd(const float* x, const int32_t* row_offset, int32_t n_seg, int32_t cols, int64_t ld, float* out, int64_t ld_out,
                          void* stream);
int echr_seg_col_mean_bwd(const float* g, int64_t ld_g, const int32_t* row_offset, int32_t n_seg, int32_t cols, int64_t ld, float* gx,
                          void* stream);
/* Non-zero initial decoder state (CG_init_feats_type) of a batch: row n of a->h0 [N, 3H] is what echr_init_state_fwd forms for event n in
 * its own video.  'V' reads x->video[vid[n], :] (a->video is ignored); 'C' divides the sum over the event's rows by the padded clip length
 * of ITS video, the largest ev_len among that video's events (a->A is ignored) -- video_len: device int32 [V] scratch, written on the
 * device by the call (may be NULL without 'C'); no host index is added.  A one-video batch equals echr_init_state_fwd bit for bit (same
 * summation order, same product).  x->ws is not read.
 * bwd: init_linear's gradients summed over all rows of all videos (written, or accumulated when `zeroed`); d event ADDED to g->g_event;
 * x->g_video [V, Dv] (optional; g->g_video is ignored) WRITTEN with the sum over the rows of each video in ascending row order -- vid is
 * non-decreasing, so a contiguous run: one fixed order, no atomics. */
int echr_init_state_fwd_batch(const echr_init_state_args* a, const echr_batch_ext* x, int32_t* video_len, void* stream);
int echr_init_state_bwd_batch(const echr_init_state_args* a, const echr_init_state_grads* g, const echr_batch_ext* x, void* stream);
int echr_tsrm_fwd_batch(const echr_tsrm_args* a, const echr_dropout* drop, const echr_batch_ext* x, void* stream);
/* (the backward kernels need no mask: the saved softmax weights of cross-video pairs are exactly 0, so d score = w * (..) is 0 there) */
int echr_tsrm_bwd_batch(const echr_tsrm_args* a, const echr_tsrm_grads* g, const echr_dropout* drop, const echr_batch_ext* x, void* stream);
/* a->prepared must be 0.  N <= 64 takes the persistent recurrences exactly as a single video does (they read the gate pre-activations,
 * which already hold the per-row scene part); with a->h0 (echr_init_state_fwd_batch's rows) the launch-per-phase ones run at every row
 * count, as for one video, and echr_decoder_bwd_batch writes g->g_h0. */
int echr_decoder_fwd_batch(const echr_dec_args* a, const echr_dropout* drop, const echr_batch_ext* x, void* stream);
/* d W_ih2[:, E:] = (sum over time and over the events of a video of d gates2)^T . video; x->g_video [V, Dv] the matching data gradient */
int echr_decoder_bwd_batch(const echr_dec_args* a, const echr_dec_grads* g, const echr_dropout* drop, const echr_batch_ext* x, void* stream);
/* Greedy decode of a batch (a->multinomial must be 0): echr_decoder_sample with per-row scene vectors (dec.h0: the per-step chain). */
int echr_decoder_sample_batch(const echr_sample_args* a, const echr_batch_ext* x, void* stream);
/* Beam search over a batch: echr_decoder_beam with per-row scene vectors.  a->dec.N = events * beam_size event-major rows as there;
 * x->vid is a device [dec.N] array in which the B rows of an event carry that event's video (non-decreasing), x->video [V, Dv], x->ws
 * echr_batch_ws_floats(dec.N, V, H) floats; dec.h0 (optional, echr_init_state_fwd_batch's rows) repeated B times per event; rows_disjoint 0.  seq, seq_logp,
 * score and words are echr_decoder_beam's; echr_beam_ws_floats sizes ws_beam.
 * video_words: device int32 [V+1] out, written behind the result on the same stream -- video_words[v] = the largest word count among
 * the events of video v (the contiguous run of events e whose row e*B has vid == v; 0 for a video without an event), video_words[V] =
 * the maximum over the batch.  Every element is written (no zero fill by the caller) and none is read by the device: the host reads
 * this vector once, instead of words[N/B], and cuts every video's rows to the width that video alone would have produced. */
int echr_decoder_beam_batch(const echr_beam_args* a, const echr_batch_ext* x, int32_t* video_words, void* stream);
/* The sampled pass of self-critical training over a batch: echr_decoder_sample_train (a->multinomial must be 1, training-mode dropout under
 * `drop` with the masks echr_decoder_fwd_batch draws at the same step, the initial state of dec.h0 or zeros, the launch-per-step chain) with per-row scene
 * vectors.  Draws are keyed (seed, batch-global row, step), so a one-video batch equals echr_decoder_sample_train bit for bit.  The
 * multinomial step is ONE launch per step: the workgroup of a row forms it from the k-slice slabs of the logits product (or reads the
 * finished logits of the many-row chain), keeps it on chip and draws -- the token and log-prob of the single-video entry's slab-sum + draw
 * pair on the same logits; vocabularies above 12 288 words stream the row instead.
 * video_words: device int32 [V+1] out, written behind the last step on the same stream (one launch, no host synchronisation) --
 * video_words[v] = the largest number of non-zero tokens among the rows of video v, i.e. the width at which that video's own call cuts its
 * output, video_words[V] = the maximum over the batch.  Every element is written and none is read by the device. */
int echr_decoder_sample_train_batch(const echr_sample_args* a, const echr_dropout* drop, const echr_batch_ext* x, int32_t* video_words,
                                    void* stream);
/* echr_train_step over a batch.  Criterion weights as in echr_train_step_rw: `weight` device [N,S] with host_nll = 0, or behind the mask
 * in host_index with host_nll = 1 (then weight = NULL).  host_index additionally ENDS with vid[N]; x->vid and x->ws are ignored (the
 * library points them at its staged copy / its own workspace).  loss[0] = the summed loss, loss[1] = sum(mask) over the batch;
 * video_loss: optional device [V] out, the per-video losses (fixed summation order).  Not with prepared, defer_update nor g_tap.  With
 * w_init (CG_init_feats_type) echr_init_state_fwd_batch / _bwd_batch run around the decoder as echr_init_state_fwd / _bwd do for one
 * video: the per-video padded clip lengths are formed on the device, the recurrences are the launch-per-phase ones at every row count.
 * handover = 1 (with do_step = 0) records both hand-over points, see echr_handover_wait (init_linear's slots lie in neither range). */
int64_t echr_train_step_batch_ws_floats(const echr_train_step_args* a, const echr_batch_ext* x);
int echr_train_step_batch(const echr_train_step_args* a, const echr_batch_ext* x, const float* weight, float* video_loss, void* stream);
/* The joint 'tap_cg' iteration over a batch: echr_train_step_batch with a->g_tap set.  g_tap [T_tot, Ht] is zero-filled by the caller and
 * added into in place: d loss / d tap of the anchors' rows through the block-diagonal event encoder (a->dec / host_index `ind` are
 * batch-absolute; 'ER1' adds nothing), and with 'VH' (a->vh_offset >= 0) each video's d scene vector spread over that video's OWN rows --
 * row_offset: device int32 [V+1] (may be NULL without 'VH').  a->g_loss (device scalar) scales every gradient, g_tap included (lambda2);
 * loss and video_loss are reported unscaled.  Not with prepared, defer_update, mid_cb nor forward_only.  With w_init and 'V', init_linear's
 * d video [V, Dv] is spread over each video's own rows like the decoder's.  handover = 1
 * (with do_step = 0) records both hand-over points (g_tap and the 'VH' span are no part of flat_g), see echr_handover_wait. */
int64_t echr_train_step_batch_tap_ws_floats(const echr_train_step_args* a, const echr_batch_ext* x);
int echr_train_step_batch_tap(const echr_train_step_args* a, const echr_batch_ext* x, const float* weight, float* video_loss,
                              const int32_t* row_offset, void* stream);
/* echr_train_step_batch with the frame-level context 'CH' / 'CC+CH' of echr_clip_step_args.  In `a`, dec.D / dec.Tv describe the ROW SOURCE
 * over the T_tot concatenated rows (D = Ht or Dc + Ht) and dec.c3d is ignored: the library takes tap itself ('CH') or forms [c3d | tap] in
 * the call's workspace ('CC+CH'); x->c3d [T_tot, Dc] feeds the event encoder.  ev_start is batch-absolute, so an event attends over rows of
 * its own video only.  Criterion weights as in echr_train_step_batch (`weight`, or behind the mask in host_index); x->rw and x->weight are
 * not read.  With a->g_tap set ([T_tot, Ht], zero-filled by the caller) it is also the joint form of echr_train_step_batch_tap: g_tap gains
 * the anchors' rows through the block-diagonal event encoder, the 'VH' span spread over each video's own rows (row_offset, device [V+1];
 * may be NULL without 'VH') and the clip-row gradient (echr_decoder_row_grad's sum; its context term reads the compacted active rows
 * directly, "row_grad_list"), all three scaled by a->g_loss, and is final when the call returns.  Not with prepared, defer_update nor
 * mid_cb, nor with an initial state that reads the clip ('C': it has no row gradient); dec.D must match clip_parts.  handover = 1 (with do_step = 0) records both hand-over points (the clip-row
 * gradient goes into g_tap, behind the join of the helper streams: no part of flat_g), see echr_handover_wait. */
int64_t echr_train_step_batch_clip_ws_floats(const echr_train_step_args* a, const echr_clip_step_args* x, const echr_batch_ext* bx);
int echr_train_step_batch_clip(const echr_train_step_args* a, const echr_clip_step_args* x, const echr_batch_ext* bx, const float* weight,
                               float* video_loss, const int32_t* row_offset, void* stream);

/* Hand-over points of the LAST one-call step issued with handover = 1 (which: 0 = logit layer, 1 = LSTM layers): makes `stream` wait
 * until that range of flat_g is final.  0 = `stream` now waits; 1 = the call recorded no such point (a configuration without the
 * asynchronous tail: the range is final when the call's own stream reaches its end, like every other); < 0 error.
 * Which entries record which points.  Both points are recorded inside the shared decoder backward, so every entry that reaches it with
 * handover = 1 and do_step = 0 records the same two: echr_train_step, echr_train_step_rw (the reward weights only change d logits),
 * echr_train_step_clip, echr_train_step_batch, echr_train_step_batch_tap and echr_train_step_batch_clip -- with the persistent and the
 * launch-per-phase recurrences, and in the fixed-order mode (its fold launches sit on the stream of the product they fold, in front of the
 * mark).  ECHR_HANDOVER_LSTM sits on the prepare stream behind the grouped weight-gradient product, the bias sums, the event half of W_ih0
 * and the scene half of W_ih2 (a batch: the segmented row sum by video and its two products); ECHR_HANDOVER_LOGIT on the tail stream behind
 * d W_logit and d b_logit.  What follows a mark writes other ranges (embedding, attention, event encoder) or no part of flat_g at all
 * (g_tap: the anchors' rows, the 'VH' span, the clip-row gradient; a batch's d video).  No point is recorded, and 1 is returned, without
 * the helper streams (LOGIT: also on the native product path without its deferred logit-layer gradients), with do_step = 1 and by the
 * deferred joint form (defer_update).  A forward_only call returns ahead of the backward pass and leaves the points of an earlier call as
 * they were (their events have long completed); echr_train_step_prepare records none. */
/* Memory scope of the library's ordering points.  echr_handover_wait's events carry a system-scope release (their consumers sit outside the
 * library: collectives read by peers, copy engines).  echr_stream_join -- and every entry that joins the helper streams by itself -- orders
 * `stream` behind the helper streams with AGENT-scope events (no cache write-back for the host or other devices: ~2 us less per edge, a dozen
 * edges per iteration): kernels queued on `stream` afterwards see every result; a consumer on another device or the host must follow the join
 * with a system-scope point of its own on `stream` -- hipStreamSynchronize, or an event created without hipEventDisableSystemFence (what
 * torch.distributed records in front of every collective).  ECHR_EVENT_SYSTEM_FENCE=1 in the environment makes every library event system-scope. */
enum { ECHR_HANDOVER_LOGIT = 0, ECHR_HANDOVER_LSTM = 1 };
int echr_handover_wait(int which, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optional per-kernel-class timing (HIP events recorded on the launch stream around every launch of the
 * class) for bench.py's roofline leg.  kind: 0 fp32 MFMA GEMM, 1 attention fwd, 2 attention bwd,
 * 3 attention post-pass, 4 recurrent grouped GEMM, 5 other, 6 bf16x3-split GEMM, 7 h2 (fp16-pair) GEMM, 8 h2 operand packing,
 * 9 persistent recurrence kernels (csrc/persist.hip).  echr_prof_read synchronises the recorded events and
 * returns the totals since echr_prof_enable(1): elapsed ms, algorithmic flops / bytes, launches.
 * Not thread-safe; never enabled on the product path.
 * ---------------------------------------------------------------------------------------------- */
int echr_prof_enable(int on);
int echr_prof_read(int kind, double* ms, double* flops, double* bytes, int64_t* launches);
/* total ms of `n` back-to-back event pairs around nothing: the fixed per-launch cost of event timing, which bench.py subtracts */
int echr_prof_event_overhead(double* ms, int64_t* n);

/* Runtime switches (defaults from the environment variables ECHR_GEMM_H2=1, ECHR_GEMM_BF16X3=1, ECHR_ATT_SLOTS=2); any other key returns -22:
 *   "gemm_h2"     0/1  run the decoder's large projections on h2-packed operands (two block-scaled fp16 planes, fp32-grade) or not
 *   "gemm_bf16x3" 0/1  (gemm_h2 = 0) use the three-plane bf16 split product for the large projections or the native fp32 MFMA
 *   "att_slots"   2/4/8 attention slots per wave
 *   "persist"     0/1  (default 1, ECHR_PERSIST) run the teacher-forced recurrence as ONE persistent launch of 256 workgroups (csrc/persist.hip:
 *                      the attention chain as two half-chip machines of 32 event rows + the two plain LSTM streams) when the shape allows
 *                      (N <= 64, A <= 258, H = Ha = 512, D <= 512, a full 256-CU device), else one launch per phase
 *   "persist_bwd" 0/1  (default 1, ECHR_PERSIST_BWD) the same for the reverse recurrence of echr_decoder_bwd (independent of "persist")
 *   "persist_h2"  0/1  (default 1, ECHR_PERSIST_H2) fp16-pair (fp32-grade) MFMA products in the forward persistent kernels (0: exact
 *                      fp32 MFMAs); the reverse kernels always use fp32 MFMAs
 *   (the switches that selected the one-machine attention chain, the two-launch pairs and the wide reverse LSTM role are retired: only
 *                      their default forms remain, and their keys return -22 like any unknown key)
 *   "persist_coop" 0/1  (default 0, ECHR_PERSIST_COOP) launch the persistent pairs with hipLaunchCooperativeKernel: the dispatch starts only
 *                      when all 256 workgroups can be co-resident, whatever else holds CUs (RCCL kernels of a data-parallel run, another
 *                      process on the device).  echr_amd.parallel / bench.py switch it on when the world size is > 1
 *   "persist_spin_limit" n  bound of every hand-off spin in polls (0 = default, about seconds; ECHR_PERSIST_SPIN_LIMIT)
 *   "persist_inject_timeout" code  diagnostic: the hand-off wait with this code (attention chain: 100000 * edge + timestep, edge 1 h1 / 2 q / 3 context / 4 d q / 5 d h / 6 d G / 7 d ATT) never completes, so the
 *                      launch aborts through its time-out path (tests/test_gpu_parity.py::test_persistent_abort_path); 0 = off
 *   "sst_persist" 0/1   (default 1, ECHR_SST_PERSIST) proposal encoder's recurrences as one persistent launch per direction (H = 512)
 *   "persist_sample" 0/1 (default 1, ECHR_PERSIST_SAMPLE) greedy decoding (echr_decoder_sample) as one persistent launch per 64 events, every step
 *                      on device (vocabularies of up to 15 360 words, the persistent forward kernel's shapes); 0 = one launch chain per step
 *   "posemb_rows" 0/1   (default 1, ECHR_POSEMB_ROWS) pairwise position embedding with one thread per frequency (contiguous stores); 0 = one
 *                      thread per 16 frequencies of a pair
 *   "posemb_packed" 0/1 (default 1, ECHR_POSEMB_PACKED) >= 4096 event pairs: the position embedding is written directly as the packed fc1 operand
 *   "persist_sample_max" n (default 512, ECHR_PERSIST_SAMPLE_MAX) greedy decoding of more than n events takes one batched launch chain per step (every
 *                      product an h2 GEMM over the N rows, fixed-order k loops: bitwise reproducible) instead of one persistent launch per 64 events;
 *                      0 = always the persistent form
 *   "persist_sample_force_eos" k  diagnostic: the persistent greedy decoder's logits of steps >= k - 1 favour <eos> for every event, so the launch takes
 *                      its early-stop path at a known step (tests); 0 = off
 *   "pair_tables" 0/1   (default 1, ECHR_PAIR_TABLES) inference over >= 16384 event pairs with known index bounds: fc1 tabulated over the distinct keys
 *   "gemm_skinny" 0/1   (default 1, ECHR_GEMM_SKINNY) the event encoder's fc2 over >= 4096 event pairs (512 -> <= 16 columns) as a streaming
 *                      16-row-tile kernel instead of the general tiles
 *   "deterministic" 0/1 (default 0, ECHR_DETERMINISTIC) fixed-order accumulation: every order-dependent fp32 sum of a training iteration is replaced
 *                      by a fixed-order one -- products run one k loop per output tile (no split-K atomics; grouped problems that share an output run
 *                      one after the other), the recurrences run launch-per-phase with the accumulator products' k-slices folded in slice order (the
 *                      persistent kernels' exchange adds are atomics: not used), column sums have one owner workgroup per 64 columns, the token
 *                      scatter-add and the anchor-row scatter have one owner per destination row and add in source order, the attention backward
 *                      writes per-chunk / per-(event, position) / per-workgroup slabs that fold launches sum in index order (scratch owned by the
 *                      library, grown on demand).  Two runs on the same inputs, parameters and dropout seed then agree bit for bit in loss and
 *                      every gradient (the reference's CPU path is run-to-run deterministic at a fixed thread count); cost: see DESIGN.md section 4h
 *   "row_grad_list" 0/1 (default 1, ECHR_ROW_GRAD_LIST) echr_train_step_batch_clip: the clip-row gradient's context term reads the compacted active
 *                      rows directly and marks an event's live steps in LDS; 0 = the flag form of the single-video entries (fill + mark + scatter).
 *                      The same sums in the same order either way
 *   "persist_stamps" 0/1/2 diagnostic phase stamps of the forward (1) / reverse (2) pair, see echr_persist_read_stamps
 *   "gemm_tile", "gemm_split"  tuning overrides of the GEMM tile / split-K heuristics (0 = heuristics; tools/gemm_bench.py only) */
int echr_config_set(const char* key, int32_t value);

/* Diagnostic (never on the product path): with echr_config_set("persist_stamps", 1) the persistent recurrence kernels record
 * s_memrealtime stamps (100 MHz) at their phase boundaries for one workgroup per role; this copies the last launch's stamps
 * ([4 roles][S][16] uint64) to host memory (synchronises the device) and returns S (0 = nothing recorded). */
/* diagnostic: role index of workgroup `block` of the merged 256-workgroup recurrence launches under placement `mode` (csrc/persist.hip,
 * persist_role_index); a bijection of 0..255 for every mode. */
int32_t echr_persist_role_index(int32_t block, int32_t mode);
int echr_persist_read_stamps(uint64_t* dst, int32_t max_entries);

/* stand-alone element-wise clamp (misc/utils.py:107-111) for optimisers other than the fused one */
int echr_clamp(float* g, int64_t n, float clip, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One-stream attention decoder: caption_model 'show_attend_tell' with CG_num_layers = 1 (the default of the reference's opts.py).
 * Replaces ShowAttendTellCore.forward (models/OldModel_NEW.py:190-274) under OldModel.forward / get_logprobs_state / the greedy branch of
 * OldModel.sample (:98-187).  Per event n and step t, from h(-1) = c(-1) = 0 or h0:
 *   q = h2att(h(t-1))  (the UNDROPPED state);  w = softmax over the event's own rows of alpha_net(tanh(ctx2att(clip) + q));  att = sum_a w_a clip_a;
 *   x = [embed(it) | video if V | event if E | att if C];  gates = x . W_ih^T + h(t-1) . W_hh^T (no bias; i, f, g, o);  LSTM cell;
 *   logp = log_softmax(logit(dropout(h(t))))     -- ONE dropout site (echr_dropout.p_out, the counter's site 4, element n * H + u, step t).
 * The state handed from step to step (and in / out of echr_sat_step) is the undropped (h, c).
 * Per step the recurrence is the attention launches of the three-stream decoder and ONE fused kernel (csrc/sat.hip): [att | h(t-1)] .
 * [W_ih[:, C columns] | W_hh]^T on the f32-input matrix cores (K = D + H, or H without 'C'), the pre-computed token / video / event rows and
 * the cell in its epilogue; the reverse pass is one kernel per step as well (d gates from the saved activations, then d [att | h(t-1)]
 * against the same panel).  Every sum has a fixed order except where the three-stream decoder's attention backward and the split-K weight
 * gradients add atomically; echr_config_set("deterministic", 1) replaces those too.  H, D, E, Ha multiples of 4; any N >= 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t N, A, Tv, D, H, E, Ha, De, Dv, V1, S;
    int32_t feats;                             /* CG_input_feats_type: bit 0 'V', bit 1 'E', bit 2 'C' (non-zero).  Fixes the columns of w_ih
                                                  behind the E token columns: [video Dv if V | event De if E | attended clip D if C] */
    int32_t rows_disjoint;                     /* 1: no two events share a video row */
    const float* embed;                        /* embed.weight [V1,E] */
    const float *w_logit, *b_logit;            /* logit [V1,H],[V1] */
    const float* w_ih;                         /* core.rnn.weight_ih_l0 [4H, E + X], X = the widths `feats` selects */
    const float* w_hh;                         /* core.rnn.weight_hh_l0 [4H, H] */
    const float *w_c2a, *b_c2a;                /* core.ctx2att [Ha,D],[Ha] */
    const float *w_h2a, *b_h2a;                /* core.h2att [Ha,H],[Ha] */
    const float *w_alpha, *b_alpha;            /* core.alpha_net [1,Ha],[1] */
    const float* c3d;                          /* [Tv,D] */
    const int32_t *ev_start, *ev_len;          /* [N] */
    const float* event;                        /* [N,De]; read with 'E' only */
    const float* video;                        /* [Dv];   read with 'V' only */
    const int32_t* tokens;                     /* [S,N] time-major input tokens */
    const float* h0;                           /* optional [N,H]: h(-1) = c(-1) = init_linear(...) (one layer); NULL = zeros */
    float* ws;                                 /* echr_sat_ws_floats; saved for echr_sat_bwd */
    float* logp;                               /* out [N,S,V1] */
    int32_t train;                             /* 1 = echr_sat_bwd will follow on this workspace (informative: the forward saves the same either way) */
} echr_sat_args;

typedef struct {
    /* parameter gradients: written, or accumulated into when `zeroed` */
    float *g_embed, *g_w_logit, *g_b_logit, *g_w_ih, *g_w_hh;
    float *g_w_c2a, *g_b_c2a, *g_w_h2a, *g_b_h2a, *g_w_alpha, *g_b_alpha;      /* bit 2 of `feats` clear: exactly zero, no attention launch */
    float* g_event;                            /* [N,De] written with 'E' only (never touched otherwise); may be NULL */
    float* g_video;                            /* [Dv] written with 'V' only; may be NULL */
    float* g_h0;                               /* [N,H] written when echr_sat_args.h0 is given; may be NULL */
    const float* g_logp;                       /* [N,S,V1] upstream gradient */
    float* ws_bwd;                             /* scratch, echr_sat_ws_bwd_floats */
    int32_t zeroed;                            /* 1: every parameter-gradient buffer arrives zero-filled (flat arena) */
} echr_sat_grads;

int64_t echr_sat_ws_floats(const echr_sat_args* a);
int64_t echr_sat_ws_bwd_floats(const echr_sat_args* a);
int echr_sat_fwd(const echr_sat_args* a, const echr_dropout* drop, void* stream);
int echr_sat_bwd(const echr_sat_args* a, const echr_sat_grads* g, const echr_dropout* drop, void* stream);
/* ONE get_logprobs_state: a->S is ignored (1), tokens = it [N], logp = out [N,V1], ws from echr_sat_ws_floats with S = 1; h / c are [1,N,H],
 * the undropped state.  drop->offset selects the dropout stream of the call (step 0 of it).  Forward only; bitwise reproducible. */
int echr_sat_step(const echr_sat_args* a, const float* h_in, const float* c_in, float* h_out, float* c_out, const echr_dropout* drop, void* stream);
/* Greedy decode: seq_len steps on device without host syncs, eval mode; seq / seq_logp / n_unfinished as the three-stream sampler's argument struct
 * defines them; ties go to the lowest index.  dec: S, tokens, logp unused; ws from echr_sat_ws_floats with S = seq_len. */
typedef struct {
    echr_sat_args dec;
    int32_t seq_len;
    int64_t* seq;            /* [N, seq_len] */
    float* seq_logp;         /* [N, seq_len] */
    int32_t* n_unfinished;   /* [seq_len + 1] */
    float* ws_sample;        /* echr_sat_sampler_ws_floats */
} echr_sat_sample_args;
int64_t echr_sat_sampler_ws_floats(const echr_sat_args* a);
int echr_sat_sample(const echr_sat_sample_args* a, void* stream);
/* The one-stream decoder over a multi-video batch, under the rules of "Multi-video batches" above: feature rows concatenated (Tv = the total
 * row count, A = the widest event of the batch), ev_start batch-absolute, vid non-decreasing, one scene vector per video, gradients the SUM
 * over the videos.  Each entry takes the arguments of its single-video sibling plus the extension:
 *   - echr_sat_args.video is ignored: row n reads x->video[vid[n], :].  The scene product is formed once per video ([V, 4H], each row with
 *     the single-video entry's arithmetic), gathered by vid on the device and added to the pre-activations per row, where the single-video
 *     entry adds its one [4H] row.  With n_videos = 1 the arithmetic and its order are the single-video entry's: a one-video batch equals
 *     echr_sat_fwd / echr_sat_sample bit for bit in eval mode;
 *   - h0 (optional): the rows echr_init_state_fwd_batch forms with H3 = H;
 *   - dropout: one counter per call; the one site is keyed by element n * H + u with n the BATCH-GLOBAL row (and step t), so row n of a
 *     batch draws what a single-video call draws for its row n only when the video is the batch's first;
 *   - backward: d W_ih[:, V columns] = sum over v of (sum over t and the rows of v of d gates)^T . video[v]; x->g_video [V, Dv] (optional;
 *     echr_sat_grads.g_video is ignored) is WRITTEN with the matching data gradient -- the rows of a video are one contiguous run of vid,
 *     added in ascending row order, no atomics.  d event, g_h0 and the other parameter gradients are per row, as for one video;
 *     "deterministic" = 1 keeps its meaning;
 *   - greedy decode: every row stops on its own <eos>; the chain runs seq_len steps and n_unfinished counts over the batch, so the caller
 *     cuts at the width of the batch's longest caption and finds each video's own width on the host from seq.
 * x->ws: echr_sat_batch_ws_floats(N, n_videos, H) floats (read with 'V' only; may be NULL otherwise), only read and written inside the
 * call.  Checked before the first launch: n_videos in [1, N], vid, and x->video with 'V'.  vid is device memory: that it does not decrease
 * is the caller's contract (echr_amd.sat checks it on the host vector it uploads). */
int64_t echr_sat_batch_ws_floats(int32_t N, int32_t n_videos, int32_t H);
int echr_sat_fwd_batch(const echr_sat_args* a, const echr_dropout* drop, const echr_batch_ext* x, void* stream);
int echr_sat_bwd_batch(const echr_sat_args* a, const echr_sat_grads* g, const echr_dropout* drop, const echr_batch_ext* x, void* stream);
int echr_sat_sample_batch(const echr_sat_sample_args* a, const echr_batch_ext* x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHR_HIP_H */
