// One-stream attention caption decoder on gfx950: caption_model 'show_attend_tell' with one LSTM layer
// (reference models/OldModel_NEW.py:190-274 under OldModel.forward / get_logprobs_state / sample, :98-187).
//
// Per step the recurrence is q = h2att(h(t-1)) (a small product), the attention score / context launches of decoder.hip, and ONE
// fused kernel: [att | h(t-1)] . [W_ih[:, C columns] | W_hh]^T on v_mfma_f32_32x32x2_f32 (exact fp32, one k-ordered fma chain per
// output: no split-K, bitwise repeatable), whose epilogue adds the token / video / event rows formed ahead of the loop, applies the
// LSTM cell and writes h, c, the dropped output and the gate activations the reverse pass reads.  The reverse pass is one kernel per
// step too: d gates from (d h, d c) and the saved activations, staged in LDS as the A operand of d [att | h(t-1)] = d gates . panel.
// Everything else (ctx2att over the video rows, token-side gate rows, logits, log-softmax, every weight gradient, the embedding
// scatter) is one product over all S*N rows through gemm.hip / core.hip.
//
// Time-major workspace [S, N, .]; HS[t] / CS[t] hold the UNDROPPED h(t-1) / c(t-1) (the state the reference hands on), OUTD the
// dropped output that feeds the logit layer -- the decoder's one dropout site.
#include <cstdint>
#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

constexpr unsigned SAT_SITE_OUT = 4;          // the counter's site of OldModel.dropout (decoder.hip SITE_OUT, echr_amd/philox.py)
typedef float sat_f32x16 __attribute__((ext_vector_type(16)));
constexpr int SKC = 64;                       // k chunk staged per round
constexpr int SLD = SKC + 4;                  // LDS row stride (floats): 16-byte aligned rows, conflict-free b128 fragment reads
constexpr int SUNITS = 16;                    // hidden units per workgroup of the forward cell: 4 gates x 16 units = one 64-column tile

#define SRC(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

__device__ __forceinline__ float4 sat_ld4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// the weight panel [W_ih[:, C columns] | W_hh]: element (gate row gr, k) for k in [0, Dc + H)
struct SatPanel {
    const float* wic; long ldw;   // W_ih + the first attended-clip column, leading dimension E + X (nullptr without 'C')
    const float* whh;             // [4H, H]
    int Dc, H;                    // D with 'C', else 0
    int vec_ic;                   // wic rows are 16-byte aligned
};
__device__ __forceinline__ float4 sat_panel4(const SatPanel& W, int gr, int k) {
    if (k < W.Dc) return sat_ld4(W.wic + (long)gr * W.ldw + k, W.vec_ic != 0);
    return *reinterpret_cast<const float4*>(W.whh + (long)gr * W.H + (k - W.Dc));
}

// ------------------------------------------------------------------------------------------------------
// forward cell.  grid (ceil(H / 16), ceil(N / 64)), 256 threads = 2 x 2 waves of 32 x 32 MFMA tiles over a [64 events] x [4 gates x 16
// units] tile; K = Dc + H walked in chunks of 64 in ONE order.  Lane l feeds MFMA j of an 8-wide k group with element j of its float4
// (k = 8c + 4 (l >> 5) + j) for both operands, as rec_gemm_kernel does.
// ------------------------------------------------------------------------------------------------------
struct SatCellFwd {
    const float* att;             // [N, Dc] attended clip of this step (unused when Dc = 0)
    const float* hprev; const float* cprev;     // [N, H]
    float* pre;                   // [N, 4H] in: token + video + event part of the pre-activations; out: the gate activations
    float* hnew; float* cnew; float* outd;      // [N, H]
    int N, t;
};
__global__ __launch_bounds__(256) void sat_cell_fwd_kernel(SatCellFwd P, SatPanel W, DropCfg dout) {
    __shared__ __attribute__((aligned(16))) float smem[2 * 64 * SLD];
    float* As = smem;
    float* Bs = smem + 64 * SLD;
    const int H = W.H, K = W.Dc + H;
    const int u0 = blockIdx.x * SUNITS, m0 = blockIdx.y * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, hh = lane >> 5;
    sat_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // the next chunk's global loads are issued ahead of this chunk's MFMA chain and land in registers meanwhile
    float4 ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int f = tid + p * 256;
            const int row = f >> 4, k = k0 + (f & 15) * 4;
            ra[p] = make_float4(0.f, 0.f, 0.f, 0.f); rb[p] = ra[p];
            const int n = m0 + row;
            if (n < P.N && k < K) ra[p] = k < W.Dc ? *reinterpret_cast<const float4*>(P.att + (long)n * W.Dc + k)
                                                   : *reinterpret_cast<const float4*>(P.hprev + (long)n * H + (k - W.Dc));
            const int u = u0 + (row & 15);
            if (u < H && k < K) rb[p] = sat_panel4(W, (row >> 4) * H + u, k);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += SKC) {
        if (k0) __syncthreads();          // the previous chunk's fragment reads are done
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int f = tid + p * 256;
            const int row = f >> 4, kq = (f & 15) * 4;
            *reinterpret_cast<float4*>(&As[row * SLD + kq]) = ra[p];
            *reinterpret_cast<float4*>(&Bs[row * SLD + kq]) = rb[p];
        }
        __syncthreads();
        if (k0 + SKC < K) fetch(k0 + SKC);
        const float* ap = &As[(wm + l31) * SLD + 4 * hh];
        const float* bp = &Bs[(wn + l31) * SLD + 4 * hh];
#pragma unroll
        for (int c = 0; c < SKC / 8; ++c) {
            const float4 a4 = *reinterpret_cast<const float4*>(ap + 8 * c);
            const float4 b4 = *reinterpret_cast<const float4*>(bp + 8 * c);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
        }
    }
    __syncthreads();
    float* Cs = smem;                      // [64][65]: the tile's products, rows = events, columns = gate * 16 + unit
#pragma unroll
    for (int r = 0; r < 16; ++r) Cs[(wm + (r & 3) + 8 * (r >> 2) + 4 * hh) * 65 + wn + l31] = acc[r];
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int idx = tid + p * 256;
        const int row = idx >> 4, ul = idx & 15;
        const int n = m0 + row, u = u0 + ul;
        if (n >= P.N || u >= H) continue;
        float* g = P.pre + (long)n * 4 * H;
        const float* cs = Cs + row * 65 + ul;
        const float gi = fast_sigmoid(g[u] + cs[0]), gf = fast_sigmoid(g[H + u] + cs[16]);
        const float gg = tanhf(g[2 * H + u] + cs[32]), go = fast_sigmoid(g[3 * H + u] + cs[48]);
        const long o = (long)n * H + u;
        const float c = gf * P.cprev[o] + gi * gg;
        const float h = go * tanhf(c);
        g[u] = gi; g[H + u] = gf; g[2 * H + u] = gg; g[3 * H + u] = go;
        P.cnew[o] = c;
        P.hnew[o] = h;
        P.outd[o] = h * drop_mult(dout, (unsigned)o, (unsigned)P.t, SAT_SITE_OUT);
    }
}

// ------------------------------------------------------------------------------------------------------
// reverse cell.  grid (ceil((Dc + H) / 64), ceil(N / 64)): a [64 events] x [64 columns of d [att | h(t-1)]] tile, contraction over the 4H
// gates in chunks of 16 units x 4 gates.  Every workgroup forms the d gates of its 64 events for the chunk in LDS (the A operand); the
// column-0 workgroups also write them (and the carried d c) out for the weight gradients.  d c / d h ping-pong between two buffers, so no
// workgroup reads what another writes in the same launch.
// ------------------------------------------------------------------------------------------------------
struct SatCellBwd {
    const float* doutd;           // [N, H] d OUTD of this step
    const float* dh; const float* dc;           // [N, H] carried in: d h(t) from step t+1, d c(t)
    const float* gates; const float* cprev; const float* cnew;
    float* dg;                    // [N, 4H] out
    float* dcn;                   // [N, H] out: d c(t-1)
    float* datt;                  // [N, Dc] out
    float* dhn;                   // [N, H] out: the recurrent part of d h(t-1)
    int N, t;
};
__global__ __launch_bounds__(256) void sat_cell_bwd_kernel(SatCellBwd P, SatPanel W, DropCfg dout) {
    __shared__ __attribute__((aligned(16))) float smem[2 * 64 * SLD];
    float* As = smem;                      // [event][gate * 16 + unit] d gates
    float* Bs = smem + 64 * SLD;           // [gate * 16 + unit][column] panel rows
    const int H = W.H, K = W.Dc + H;
    const int c0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l31 = lane & 31, hh = lane >> 5;
    sat_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // the next chunk's global loads (the cell's saved values and the panel rows) are issued ahead of this chunk's MFMA chain
    float rv[4][9];          // d OUTD, d h, d c, i, f, g, o, c(t), c(t-1) of the thread's four (event, unit) pairs
    float4 rb[4];
    auto fetch = [&](int ub) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = tid + p * 256;
            const int n = m0 + (idx >> 4), u = ub + (idx & 15);
#pragma unroll
            for (int i = 0; i < 9; ++i) rv[p][i] = 0.f;
            if (n < P.N && u < H) {
                const long o = (long)n * H + u;
                const float* g = P.gates + (long)n * 4 * H;
                rv[p][0] = P.doutd[o]; rv[p][1] = P.dh[o]; rv[p][2] = P.dc[o];
                rv[p][3] = g[u]; rv[p][4] = g[H + u]; rv[p][5] = g[2 * H + u]; rv[p][6] = g[3 * H + u];
                rv[p][7] = P.cnew[o]; rv[p][8] = P.cprev[o];
            }
            const int kk = idx >> 4, ku = ub + (kk & 15), col = c0 + (idx & 15) * 4;
            rb[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ku < H && col < K) rb[p] = sat_panel4(W, (kk >> 4) * H + ku, col);
        }
    };
    fetch(0);
    for (int ub = 0; ub < H; ub += SUNITS) {
        if (ub) __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = tid + p * 256;
            const int row = idx >> 4, ul = idx & 15;
            const int n = m0 + row, u = ub + ul;
            float di = 0.f, df = 0.f, dgg = 0.f, dov = 0.f;
            if (n < P.N && u < H) {
                const long o = (long)n * H + u;
                const float dhv = rv[p][0] * drop_mult(dout, (unsigned)o, (unsigned)P.t, SAT_SITE_OUT) + rv[p][1];
                const float gi = rv[p][3], gf = rv[p][4], gg = rv[p][5], go = rv[p][6];
                const float tc = tanhf(rv[p][7]);
                const float dcv = dhv * go * (1.f - tc * tc) + rv[p][2];
                di = dcv * gg * gi * (1.f - gi);
                df = dcv * rv[p][8] * gf * (1.f - gf);
                dgg = dcv * gi * (1.f - gg * gg);
                dov = dhv * tc * go * (1.f - go);
                if (blockIdx.x == 0) {
                    float* dgo = P.dg + (long)n * 4 * H;
                    dgo[u] = di; dgo[H + u] = df; dgo[2 * H + u] = dgg; dgo[3 * H + u] = dov;
                    P.dcn[o] = dcv * gf;
                }
            }
            float* ar = As + row * SLD + ul;
            ar[0] = di; ar[16] = df; ar[32] = dgg; ar[48] = dov;
            *reinterpret_cast<float4*>(&Bs[row * SLD + ul * 4]) = rb[p];          // (panel row kk = idx >> 4, columns 4 (idx & 15) ..)
        }
        __syncthreads();
        if (ub + SUNITS < H) fetch(ub + SUNITS);
        const float* ap = &As[(wm + l31) * SLD + 4 * hh];
        const float* bp = &Bs[(4 * hh) * SLD + wn + l31];
#pragma unroll
        for (int c = 0; c < SKC / 8; ++c) {
            const float4 a4 = *reinterpret_cast<const float4*>(ap + 8 * c);
            const float* bq = bp + 8 * c * SLD;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, bq[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, bq[SLD], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, bq[2 * SLD], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, bq[3 * SLD], acc, 0, 0, 0);
        }
    }
    const int col = c0 + wn + l31;
    if (col < K) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (n < P.N) {
                if (col < W.Dc) P.datt[(long)n * W.Dc + col] = acc[r];
                else P.dhn[(long)n * H + (col - W.Dc)] = acc[r];
            }
        }
    }
}

__global__ __launch_bounds__(256) void sat_add2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}
__global__ __launch_bounds__(256) void sat_acc_kernel(float* __restrict__ dst, const float* __restrict__ src, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

// ------------------------------------------------------------------------------------------------------
// workspaces
// ------------------------------------------------------------------------------------------------------
static inline long srup(long x, long a) { return (x + a - 1) / a * a; }
struct SatDims {
    bool v, e, c;
    int cv, ce, cc;               // first column of the video / event / attended-clip part of w_ih
    int ldw, Dc;
};
static SatDims sat_dims(const echr_sat_args* a) {
    SatDims d;
    d.v = (a->feats & 1) != 0; d.e = (a->feats & 2) != 0; d.c = (a->feats & 4) != 0;
    d.cv = a->E;
    d.ce = d.cv + (d.v ? a->Dv : 0);
    d.cc = d.ce + (d.e ? a->De : 0);
    d.ldw = d.cc + (d.c ? a->D : 0);
    d.Dc = d.c ? a->D : 0;
    return d;
}
struct SatWs { float *XT, *PRE, *EVC, *VB, *HS, *CS, *OUTD, *PALL, *Q1, *QS, *SC, *WT, *ATT; long total; };
static SatWs sat_carve(const echr_sat_args* a, float* base) {
    SatWs w;
    long off = 0;
    const long N = a->N, S = a->S, H = a->H;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += srup(n, 64); return p; };
    w.XT = take(S * N * a->E);
    w.PRE = take(S * N * 4 * H);
    w.EVC = take(N * 4 * H);
    w.VB = take(4 * H);
    w.HS = take((S + 1) * N * H);
    w.CS = take((S + 1) * N * H);
    w.OUTD = take(S * N * H);
    w.PALL = take((long)a->Tv * a->Ha);
    w.Q1 = take(N * a->Ha);
    w.QS = take(S * N * a->Ha);
    w.SC = take(S * N * a->A);
    w.WT = take(S * N * a->A);
    w.ATT = take(S * N * a->D);
    w.total = off;
    return w;
}
struct SatWsB { float *DLG, *DOUT, *DG, *DGSUM, *DGCOL, *DATT, *DSC, *DXT, *DHB[2], *DCB[2], *DQ, *GAREP, *GBREP, *DPALL, *GEMB; long ldg, zero_floats, total; };
static SatWsB sat_carve_bwd(const echr_sat_args* a, float* base) {
    SatWsB w;
    long off = 0;
    const long N = a->N, S = a->S, H = a->H;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += srup(n, 64); return p; };
    w.ldg = srup(a->V1, 4);
    w.DLG = take(S * N * w.ldg);
    w.DOUT = take(S * N * H);
    w.DG = take(S * N * 4 * H);
    w.DGSUM = take(N * 4 * H);
    w.DGCOL = take(4 * H);
    w.DATT = take(N * a->D);
    w.DSC = take(S * N * a->A);
    w.DXT = take(S * N * a->E);
    w.DHB[1] = take(N * H); w.DCB[1] = take(N * H);
    // one contiguous zero-filled range: the carried d h / d c of the last step, and what the attention backward adds into
    const long z0 = off;
    w.DHB[0] = take(N * H); w.DCB[0] = take(N * H);
    w.DQ = take(S * N * a->Ha);
    w.GAREP = take((long)att_post_replicas() * a->Ha);
    w.GBREP = take(att_post_replicas());
    w.DPALL = take((long)a->Tv * a->Ha);
    w.zero_floats = off - z0;
    // the table gradient of one call, summed from zero and added to g_embed ONCE (`zeroed` = 1 only): the scatter adds a row per occurrence of
    // its token, which rounds at the magnitude of whatever the caller's buffer already holds
    w.GEMB = take((long)a->V1 * a->E);
    w.total = off;
    return w;
}

// Multi-video batches: the caller's scratch echr_batch_ext.ws = VIDV [V, 4H] (scene part of the gates per video) | VIDB [N, 4H] (gathered by vid:
// per event) | DGSEG [V, 4H] (d gates summed over time and over the events of a video)
struct SatBatchWs { float *VIDV, *VIDB, *DGSEG; long total; };
static SatBatchWs sat_carve_batch(long N, long V, long H, float* base) {
    SatBatchWs w;
    long off = 0;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += srup(n, 64); return p; };
    w.VIDV = take(V * 4 * H); w.VIDB = take(N * 4 * H); w.DGSEG = take(V * 4 * H);
    w.total = off;
    return w;
}

// bx: a multi-video batch -- a->video is not read then ('V' needs bx->video [V, Dv])
static int sat_check(const echr_sat_args* a, const char* who, const echr_batch_ext* bx = nullptr) {
    ECHR_REQUIRE(a, "%s: null args", who);
    ECHR_REQUIRE(a->N > 0 && a->A > 0 && a->Tv > 0 && a->S >= 0, "%s: bad N/A/Tv/S", who);
    ECHR_REQUIRE((a->feats & 7) != 0 && (a->feats & ~7) == 0, "%s: feats must select at least one of V (1), E (2), C (4): got %d (the reference fails on "
                 "an empty CG_input_feats_type too)", who, a->feats);
    SRC(att_check_dims(AttShape{a->N, a->A, a->Ha, a->D}, who));
    ECHR_REQUIRE(a->H > 0 && a->E > 0 && a->V1 > 1 && a->H % 4 == 0 && a->E % 4 == 0, "%s: need H%%4==0 and E%%4==0, V1 > 1 (H=%d E=%d V1=%d)", who, a->H, a->E, a->V1);
    ECHR_REQUIRE(bx || !(a->feats & 1) || (a->Dv > 0 && a->video), "%s: 'V' needs video [Dv]", who);
    ECHR_REQUIRE(!(a->feats & 2) || (a->De > 0 && a->event), "%s: 'E' needs event [N,De]", who);
    ECHR_REQUIRE(a->embed && a->w_logit && a->b_logit && a->w_ih && a->w_hh && a->w_c2a && a->b_c2a && a->w_h2a && a->b_h2a && a->w_alpha && a->b_alpha &&
                 a->c3d && a->ev_start && a->ev_len, "%s: missing parameters / inputs", who);
    ECHR_REQUIRE((uintptr_t)a->w_hh % 16 == 0, "%s: w_hh must be 16-byte aligned", who);
    return 0;
}
// the batch extension, ahead of every other check and of the first launch.  (vid lives on the device: that it does not decrease is the caller's contract, which
// echr_amd.sat checks on the host copy it builds the device vector from)
static int sat_check_batch(const echr_sat_args* a, const echr_batch_ext* x, const char* who) {
    ECHR_REQUIRE(a && x, "%s: null args / batch extension", who);
    ECHR_REQUIRE(x->n_videos >= 1 && x->n_videos <= a->N, "%s: the batch extension needs 1 <= n_videos <= N (n_videos=%d N=%d)", who, x->n_videos, a->N);
    ECHR_REQUIRE(x->vid, "%s: the batch extension needs vid [N]", who);
    if (a->feats & 1) {
        ECHR_REQUIRE(a->Dv > 0 && x->video, "%s: 'V' needs the batch's video [n_videos, Dv]", who);
        ECHR_REQUIRE(x->ws, "%s: 'V' needs the batch scratch ws (echr_sat_batch_ws_floats)", who);
    }
    return 0;
}
static SatPanel sat_panel(const echr_sat_args* a, const SatDims& d) {
    SatPanel W;
    W.wic = d.c ? a->w_ih + d.cc : nullptr; W.ldw = d.ldw; W.whh = a->w_hh; W.Dc = d.Dc; W.H = a->H;
    W.vec_ic = (d.c && d.ldw % 4 == 0 && (uintptr_t)(a->w_ih + d.cc) % 16 == 0) ? 1 : 0;
    return W;
}

// P_all = ctx2att over the video rows ('C'), and the per-event constant part of the pre-activations: EVC [N, 4H] = [video | event] .
// W_ih[:, V / E columns]^T ('E'), or the one row VB [4H] ('V' alone)
//
// Multi-video batch (bx): the scene product once per video, VIDV [V, 4H], each row with row_matvec's arithmetic (rows_matvec), gathered by
// vid into VIDB [N, 4H]; that per-row addend stands where the one-video call has the bias VB -- the same add at the same place, so a
// one-video batch forms the one-video call's values.  Returns in *rowadd what sat_token_rows adds per event (nullptr: VB, or nothing).
static int sat_static(const echr_sat_args* a, const SatDims& dm, const SatWs& w, const echr_batch_ext* bx, const float** rowadd, hipStream_t st) {
    const int H = a->H;
    echr_gemm_desc d;
    if (dm.c) {
        d = desc_nt(a->c3d, a->D, a->w_c2a, a->D, w.PALL, a->Ha, a->Tv, a->Ha, a->D);
        d.bias = a->b_c2a; d.algo = ECHR_GEMM_BF16X3;          // (three exact bf16 planes, fp32-accurate: the three-stream decoder's choice for this product)
        SRC(gemm(d, st));
    }
    const float* vidb = nullptr;
    if (dm.v && bx) {
        const SatBatchWs bw = sat_carve_batch(a->N, bx->n_videos, H, bx->ws);
        SRC(rows_matvec(bx->video, a->Dv, a->w_ih + dm.cv, dm.ldw, nullptr, nullptr, bw.VIDV, 4 * H, bx->n_videos, 4 * H, a->Dv, st));
        SRC(embed_gather(bw.VIDV, bx->vid, bw.VIDB, a->N, 4 * H, bx->n_videos, st));
        vidb = bw.VIDB;
    } else if (dm.v) SRC(row_matvec(a->video, a->w_ih + dm.cv, dm.ldw, nullptr, nullptr, w.VB, 4 * H, a->Dv, st));
    if (dm.e) {
        d = desc_nt(a->event, a->De, a->w_ih + dm.ce, dm.ldw, w.EVC, 4 * H, a->N, 4 * H, a->De);
        if (vidb) { d.addend = vidb; d.add_mod = a->N; d.ld_add = 4 * H; }
        else if (dm.v) d.bias = w.VB;
        SRC(gemm(d, st));
    }
    *rowadd = dm.e ? w.EVC : vidb;
    return 0;
}
// token-side gate rows of `rows` = nt * N token rows (embedded in xt) into PRE rows [row0, row0 + rows), plus the constant part
static int sat_token_rows(const echr_sat_args* a, const SatDims& dm, const SatWs& w, const float* rowadd, const float* xt, long row0, int rows,
                          hipStream_t st) {
    const int H = a->H;
    echr_gemm_desc d = desc_nt(xt, a->E, a->w_ih, dm.ldw, w.PRE + row0 * 4 * H, 4 * H, rows, 4 * H, a->E);
    if (rowadd) { d.addend = rowadd; d.add_mod = a->N; d.ld_add = 4 * H; }
    else if (dm.v) d.bias = w.VB;
    return gemm(d, st);
}
// one step: HS[t], CS[t], PRE[t] -> HS[t+1], CS[t+1], OUTD[t] (and QS / SC / WT / ATT [t] with 'C')
static int sat_step(const echr_sat_args* a, const SatDims& dm, const SatWs& w, int t, const DropCfg& dout, hipStream_t st) {
    const int N = a->N, H = a->H, Ha = a->Ha, A = a->A, D = a->D;
    const long hs = (long)N * H;
    const float* hprev = w.HS + (long)t * hs;
    float* att = w.ATT + (long)t * N * D;
    if (dm.c) {
        echr_gemm_desc d = desc_nt(hprev, H, a->w_h2a, H, w.Q1, Ha, N, Ha, H);          // (its bias is added by the score kernel)
        SRC(gemm(d, st));
        const AttShape as{N, A, Ha, D};
        float* sc = w.SC + (long)t * N * A;
        SRC(att_score_launch(as, w.PALL, w.Q1, a->b_h2a, w.QS + (long)t * N * Ha, a->w_alpha, a->b_alpha, a->ev_start, a->ev_len, sc, st));
        SRC(att_context_launch(as, a->c3d, sc, a->ev_start, a->ev_len, w.WT + (long)t * N * A, att, st));
    }
    SatCellFwd P;
    P.att = att; P.hprev = hprev; P.cprev = w.CS + (long)t * hs;
    P.pre = w.PRE + (long)t * N * 4 * H;
    P.hnew = w.HS + (long)(t + 1) * hs; P.cnew = w.CS + (long)(t + 1) * hs; P.outd = w.OUTD + (long)t * hs;
    P.N = N; P.t = t;
    // (optional device-event timing, off on the product path: kind PROF_LSTM counts this decoder's two cell kernels and nothing else of it)
    const double K = dm.Dc + H;
    ProfScope prof(PROF_LSTM, 2.0 * N * 4 * H * K, 4.0 * (4.0 * H * K + N * K + N * 12.0 * H), st);
    hipLaunchKernelGGL(sat_cell_fwd_kernel, dim3((H + SUNITS - 1) / SUNITS, (N + 63) / 64), dim3(256), 0, st, P, sat_panel(a, dm), dout);
    return check_launch("sat_cell_fwd");
}
static int sat_initial_state(const echr_sat_args* a, const SatWs& w, const float* h, const float* c, hipStream_t st) {
    const long hs = (long)a->N * a->H;
    if (!h) {
        float* zp[2] = {w.HS, w.CS};
        long zn[2] = {hs, hs};
        return fill_zero_multi(zp, zn, 2, st);
    }
    if (hipMemcpyAsync(w.HS, h, hs * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(w.CS, c, hs * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("sat: state copy failed"); return -5; }
    return 0;
}

}  // namespace echr

using namespace echr;

extern "C" int64_t echr_sat_ws_floats(const echr_sat_args* a) { return a ? sat_carve(a, nullptr).total : -1; }
extern "C" int64_t echr_sat_ws_bwd_floats(const echr_sat_args* a) { return a ? sat_carve_bwd(a, nullptr).total : -1; }

extern "C" int64_t echr_sat_batch_ws_floats(int32_t N, int32_t n_videos, int32_t H) {
    return (N > 0 && n_videos > 0 && H > 0) ? sat_carve_batch(N, n_videos, H, nullptr).total : -1;
}

// echr_sat_fwd (bx = nullptr) and echr_sat_fwd_batch
static int sat_fwd(const echr_sat_args* a, const echr_dropout* drop, const echr_batch_ext* bx, const char* who, void* stream) {
    if (bx) SRC(sat_check_batch(a, bx, who));
    SRC(sat_check(a, who, bx));
    ECHR_REQUIRE(a->S > 0 && a->ws && a->logp && a->tokens, "%s: missing buffers", who);
    SRC(persist_check_async());
    SRC(join_tail((hipStream_t)stream));
    hipStream_t st = (hipStream_t)stream;
    const SatDims dm = sat_dims(a);
    const SatWs w = sat_carve(a, a->ws);
    const int N = a->N, S = a->S, H = a->H;
    const DropCfg dout = make_drop(drop, drop ? drop->p_out : 0.f);
    const float* rowadd = nullptr;
    SRC(sat_initial_state(a, w, a->h0, a->h0, st));
    SRC(sat_static(a, dm, w, bx, &rowadd, st));
    SRC(embed_gather(a->embed, a->tokens, w.XT, S * N, a->E, a->V1, st));
    SRC(sat_token_rows(a, dm, w, rowadd, w.XT, 0, S * N, st));
    for (int t = 0; t < S; ++t) SRC(sat_step(a, dm, w, t, dout, st));
    echr_gemm_desc d = desc_nt(w.OUTD, H, a->w_logit, H, a->logp, a->V1, S * N, a->V1, H);
    d.bias = a->b_logit; d.rowmap_mod = N; d.rowmap_mul = S; d.algo = ECHR_GEMM_BF16X3;
    SRC(gemm(d, st));
    return logsoftmax_rows(a->logp, a->V1, N, S, 0, S, a->V1, st);
}
extern "C" int echr_sat_fwd(const echr_sat_args* a, const echr_dropout* drop, void* stream) { return sat_fwd(a, drop, nullptr, "sat_fwd", stream); }
extern "C" int echr_sat_fwd_batch(const echr_sat_args* a, const echr_dropout* drop, const echr_batch_ext* x, void* stream) {
    ECHR_REQUIRE(x, "sat_fwd_batch: null batch extension");
    return sat_fwd(a, drop, x, "sat_fwd_batch", stream);
}

extern "C" int echr_sat_step(const echr_sat_args* a0, const float* h_in, const float* c_in, float* h_out, float* c_out, const echr_dropout* drop,
                             void* stream) {
    SRC(sat_check(a0, "sat_step"));
    ECHR_REQUIRE(a0->ws && a0->logp && a0->tokens && h_in && c_in && h_out && c_out, "sat_step: missing buffers");
    SRC(persist_check_async());
    SRC(join_tail((hipStream_t)stream));
    DeterministicScope det;
    echr_sat_args a = *a0;
    a.S = 1;
    hipStream_t st = (hipStream_t)stream;
    const SatDims dm = sat_dims(&a);
    const SatWs w = sat_carve(&a, a.ws);
    const int N = a.N, H = a.H;
    const long hs = (long)N * H;
    const float* rowadd = nullptr;
    SRC(sat_initial_state(&a, w, h_in, c_in, st));
    SRC(sat_static(&a, dm, w, nullptr, &rowadd, st));
    SRC(embed_gather(a.embed, a.tokens, w.XT, N, a.E, a.V1, st));
    SRC(sat_token_rows(&a, dm, w, rowadd, w.XT, 0, N, st));
    SRC(sat_step(&a, dm, w, 0, make_drop(drop, drop ? drop->p_out : 0.f), st));
    echr_gemm_desc d = desc_nt(w.OUTD, H, a.w_logit, H, a.logp, a.V1, N, a.V1, H);
    d.bias = a.b_logit;
    SRC(gemm(d, st));
    SRC(logsoftmax_rows(a.logp, a.V1, N, 1, 0, 1, a.V1, st));
    if (hipMemcpyAsync(h_out, w.HS + hs, hs * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(c_out, w.CS + hs, hs * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("sat_step: state copy failed"); return -5; }
    return 0;
}

// sampler scratch: the step's tokens and unfinished flags, its logits
struct SatSampWs { int *IT, *UNF; float* LOGITS; long total; };
static SatSampWs sat_carve_samp(const echr_sat_args* a, float* base) {
    SatSampWs s;
    long off = 0;
    auto take = [&](long n) { float* p = base ? base + off : nullptr; off += srup(n, 64); return p; };
    s.IT = reinterpret_cast<int*>(take(a->N));
    s.UNF = reinterpret_cast<int*>(take(a->N));
    s.LOGITS = take((long)a->N * a->V1);
    s.total = off;
    return s;
}
extern "C" int64_t echr_sat_sampler_ws_floats(const echr_sat_args* a) { return a ? sat_carve_samp(a, nullptr).total : -1; }

// echr_sat_sample (bx = nullptr) and echr_sat_sample_batch: every row stops on its own <eos>, the chain runs seq_len steps either way
static int sat_sample(const echr_sat_sample_args* sa, const echr_batch_ext* bx, const char* who, void* stream) {
    ECHR_REQUIRE(sa, "%s: null args", who);
    if (bx) SRC(sat_check_batch(&sa->dec, bx, who));
    SRC(sat_check(&sa->dec, who, bx));
    const int L = sa->seq_len;
    ECHR_REQUIRE(L > 0 && sa->seq && sa->seq_logp && sa->n_unfinished && sa->ws_sample && sa->dec.ws, "%s: missing buffers", who);
    SRC(persist_check_async());
    SRC(join_tail((hipStream_t)stream));
    DeterministicScope det;                    // `seq` is an index output: one fixed-order k loop per tile everywhere
    echr_sat_args a = sa->dec;
    a.S = L;
    hipStream_t st = (hipStream_t)stream;
    const SatDims dm = sat_dims(&a);
    const SatWs w = sat_carve(&a, a.ws);
    const SatSampWs s = sat_carve_samp(&a, sa->ws_sample);
    const int N = a.N, H = a.H;
    {
        float* zp[4] = {reinterpret_cast<float*>(sa->n_unfinished), reinterpret_cast<float*>(s.IT), reinterpret_cast<float*>(sa->seq), sa->seq_logp};
        long zn[4] = {L + 1, 2L * srup(N, 64), 2L * N * L, (long)N * L};          // (IT | UNF are adjacent)
        SRC(fill_zero_multi(zp, zn, 4, st));
    }
    const float* rowadd = nullptr;
    SRC(sat_initial_state(&a, w, a.h0, a.h0, st));
    SRC(sat_static(&a, dm, w, bx, &rowadd, st));
    const DropCfg none = make_drop(nullptr, 0.f);
    for (int t = 0; t < L; ++t) {
        SRC(embed_gather(a.embed, s.IT, w.XT, N, a.E, a.V1, st));
        SRC(sat_token_rows(&a, dm, w, rowadd, w.XT, (long)t * N, N, st));
        SRC(sat_step(&a, dm, w, t, none, st));
        echr_gemm_desc d = desc_nt(w.OUTD + (long)t * N * H, H, a.w_logit, H, s.LOGITS, a.V1, N, a.V1, H);
        d.bias = a.b_logit;
        SRC(gemm(d, st));
        SRC(greedy_step(s.LOGITS, a.V1, N, a.V1, t, L, s.IT, s.UNF, reinterpret_cast<long long*>(sa->seq), sa->seq_logp, sa->n_unfinished, st));
    }
    return 0;
}
extern "C" int echr_sat_sample(const echr_sat_sample_args* sa, void* stream) { return sat_sample(sa, nullptr, "sat_sample", stream); }
extern "C" int echr_sat_sample_batch(const echr_sat_sample_args* sa, const echr_batch_ext* x, void* stream) {
    ECHR_REQUIRE(x, "sat_sample_batch: null batch extension");
    return sat_sample(sa, x, "sat_sample_batch", stream);
}

// echr_sat_bwd (bx = nullptr) and echr_sat_bwd_batch
static int sat_bwd(const echr_sat_args* a, const echr_sat_grads* g, const echr_dropout* drop, const echr_batch_ext* bx, const char* who, void* stream) {
    if (bx) SRC(sat_check_batch(a, bx, who));
    SRC(sat_check(a, who, bx));
    ECHR_REQUIRE(g && a->S > 0 && a->ws && a->logp && a->tokens && g->g_logp && g->ws_bwd, "%s: missing buffers", who);
    ECHR_REQUIRE(g->g_embed && g->g_w_logit && g->g_b_logit && g->g_w_ih && g->g_w_hh && g->g_w_c2a && g->g_b_c2a && g->g_w_h2a && g->g_b_h2a &&
                 g->g_w_alpha && g->g_b_alpha, "%s: missing parameter-gradient buffers", who);
    SRC(persist_check_async());
    SRC(join_tail((hipStream_t)stream));
    hipStream_t st = (hipStream_t)stream;
    const SatDims dm = sat_dims(a);
    const SatWs w = sat_carve(a, a->ws);
    const SatWsB b = sat_carve_bwd(a, g->ws_bwd);
    const int N = a->N, S = a->S, H = a->H, E = a->E, Ha = a->Ha, A = a->A, D = a->D, V1 = a->V1;
    const int SN = S * N, H4 = 4 * H;
    const long hs = (long)N * H;
    const DropCfg dout = make_drop(drop, drop ? drop->p_out : 0.f);
    echr_gemm_desc d;
    // scratch that is added into; without `zeroed` the parameter gradients too (everything below accumulates)
    SRC(fill_zero(b.DHB[0], b.zero_floats, st));
    if (!g->zeroed) {
        float* zp[11] = {g->g_embed, g->g_w_logit, g->g_b_logit, g->g_w_ih, g->g_w_hh, g->g_w_c2a, g->g_b_c2a, g->g_w_h2a, g->g_b_h2a, g->g_w_alpha, g->g_b_alpha};
        long zn[11] = {(long)V1 * E, (long)V1 * H, V1, (long)H4 * dm.ldw, (long)H4 * H, (long)Ha * D, Ha, (long)Ha * H, Ha, Ha, 1};
        SRC(fill_zero_multi(zp, zn, 6, st));
        SRC(fill_zero_multi(zp + 6, zn + 6, 5, st));
    }
    // 1. d logits (time-major rows, padded leading dimension), the logit layer's gradients, d OUTD
    SRC(logsoftmax_bwd(a->logp, g->g_logp, nullptr, 0, nullptr, nullptr, nullptr, b.DLG, b.ldg, N, S, V1, st));
    d = desc_tn(b.DLG, b.ldg, w.OUTD, H, g->g_w_logit, H, V1, H, SN);
    d.beta = 1.f; d.split_k = -1;
    SRC(gemm(d, st));
    SRC(colsum(b.DLG, b.ldg, SN, V1, g->g_b_logit, true, st));
    d = desc_nn(b.DLG, b.ldg, a->w_logit, H, b.DOUT, H, SN, H, V1);
    d.split_k = -1;
    SRC(gemm(d, st));
    // 2. reverse recurrence
    const SatPanel W = sat_panel(a, dm);
    const AttShape as{N, A, Ha, D};
    int cur = 0;
    for (int t = S - 1; t >= 0; --t) {
        SatCellBwd P;
        P.doutd = b.DOUT + (long)t * hs; P.dh = b.DHB[cur]; P.dc = b.DCB[cur];
        P.gates = w.PRE + (long)t * N * H4; P.cprev = w.CS + (long)t * hs; P.cnew = w.CS + (long)(t + 1) * hs;
        P.dg = b.DG + (long)t * N * H4; P.dcn = b.DCB[cur ^ 1]; P.datt = b.DATT; P.dhn = b.DHB[cur ^ 1];
        P.N = N; P.t = t;
        {
            const double K = dm.Dc + H;
            ProfScope prof(PROF_LSTM, 2.0 * N * H4 * K, 4.0 * ((double)H4 * K + N * K + N * 12.0 * H), st);
            hipLaunchKernelGGL(sat_cell_bwd_kernel, dim3((dm.Dc + H + 63) / 64, (N + 63) / 64), dim3(256), 0, st, P, W, dout);
            SRC(check_launch("sat_cell_bwd"));
        }
        if (dm.c) {
            float* dq = b.DQ + (long)t * N * Ha;
            SRC(att_bwd_launch(as, w.PALL, a->c3d, w.QS + (long)t * N * Ha, a->w_alpha, w.WT + (long)t * N * A, w.ATT + (long)t * N * D, b.DATT,
                               a->ev_start, a->ev_len, b.DSC + (long)t * N * A, dq, st));
            d = desc_nn(dq, Ha, a->w_h2a, H, b.DHB[cur ^ 1], H, N, H, Ha);          // d h(t-1) += d q . W_h2a
            d.beta = 1.f;
            SRC(gemm(d, st));
        }
        cur ^= 1;
    }
    if (a->h0 && g->g_h0) {          // h0 is both h(-1) and c(-1)
        hipLaunchKernelGGL(sat_add2_kernel, dim3((unsigned)((hs + 255) / 256)), dim3(256), 0, st, b.DHB[cur], b.DCB[cur], g->g_h0, hs);
        SRC(check_launch("sat_add2"));
    }
    // 3. weight gradients: one product over the S*N rows each.  HS[t] holds h(t-1), so its rows pair with DG[t]
    d = desc_tn(b.DG, H4, w.HS, H, g->g_w_hh, H, H4, H, SN);
    d.beta = 1.f; d.split_k = -1;
    SRC(gemm(d, st));
    d = desc_tn(b.DG, H4, w.XT, E, g->g_w_ih, dm.ldw, H4, E, SN);
    d.beta = 1.f; d.split_k = -1;
    SRC(gemm(d, st));
    if (dm.c) {
        d = desc_tn(b.DG, H4, w.ATT, D, g->g_w_ih + dm.cc, dm.ldw, H4, D, SN);
        d.beta = 1.f; d.split_k = -1;
        SRC(gemm(d, st));
    }
    if (dm.v || dm.e) SRC(sum_over_time(b.DG, H4, S, N, H4, b.DGSUM, H4, st));
    if (dm.e) {
        d = desc_tn(b.DGSUM, H4, a->event, a->De, g->g_w_ih + dm.ce, dm.ldw, H4, a->De, N);
        d.beta = 1.f; d.split_k = -1;
        SRC(gemm(d, st));
        if (g->g_event) {
            d = desc_nn(b.DGSUM, H4, a->w_ih + dm.ce, dm.ldw, g->g_event, a->De, N, a->De, H4);
            SRC(gemm(d, st));
        }
    }
    if (dm.v && bx) {
        // the rows of a video are one contiguous run of vid: summed in ascending row order (no atomics), then two products with K = V / 4H,
        // each one fixed-order k loop per tile
        const int V = bx->n_videos;
        float* dgseg = sat_carve_batch(N, V, H, bx->ws).DGSEG;
        SRC(seg_rowsum(b.DGSUM, bx->vid, N, V, H4, H4, dgseg, st));
        d = desc_tn(dgseg, H4, bx->video, a->Dv, g->g_w_ih + dm.cv, dm.ldw, H4, a->Dv, V);
        d.beta = 1.f; d.split_k = 1;
        SRC(gemm(d, st));
        if (bx->g_video) {
            d = desc_nn(dgseg, H4, a->w_ih + dm.cv, dm.ldw, bx->g_video, a->Dv, V, a->Dv, H4);
            d.split_k = 1;
            SRC(gemm(d, st));
        }
    } else if (dm.v) {
        SRC(colsum(b.DGSUM, H4, N, H4, b.DGCOL, false, st));
        SRC(rank1_update(b.DGCOL, a->video, g->g_w_ih + dm.cv, dm.ldw, H4, a->Dv, true, st));
        if (g->g_video) SRC(vec_mat(b.DGCOL, a->w_ih + dm.cv, dm.ldw, g->g_video, H4, a->Dv, st));
    }
    if (dm.c) {
        d = desc_tn(b.DQ, Ha, w.HS, H, g->g_w_h2a, H, Ha, H, SN);
        d.beta = 1.f; d.split_k = -1;
        SRC(gemm(d, st));
        SRC(colsum(b.DQ, Ha, SN, Ha, g->g_b_h2a, true, st));
        SRC(att_post_launch(as, a->Tv, S, a->rows_disjoint, w.PALL, w.QS, a->w_alpha, b.DSC, a->ev_start, a->ev_len, b.DPALL, b.GAREP, b.GBREP,
                            g->g_w_alpha, g->g_b_alpha, st));
        d = desc_tn(b.DPALL, Ha, a->c3d, D, g->g_w_c2a, D, Ha, D, a->Tv);
        d.beta = 1.f; d.split_k = -1;
        SRC(gemm(d, st));
        SRC(colsum(b.DPALL, Ha, a->Tv, Ha, g->g_b_c2a, true, st));
    }
    // 4. token embedding: d XT = DG . W_ih[:, :E], scatter-added into the table gradient
    d = desc_nn(b.DG, H4, a->w_ih, dm.ldw, b.DXT, E, SN, E, H4);
    SRC(gemm(d, st));
    if (!g->zeroed) return embed_scatter_add(b.DXT, a->tokens, g->g_embed, SN, E, V1, st);          // (zero-filled above)
    const long ne = (long)V1 * E;
    SRC(fill_zero(b.GEMB, ne, st));
    SRC(embed_scatter_add(b.DXT, a->tokens, b.GEMB, SN, E, V1, st));
    hipLaunchKernelGGL(sat_acc_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, g->g_embed, b.GEMB, ne);
    return check_launch("sat_acc");
}
extern "C" int echr_sat_bwd(const echr_sat_args* a, const echr_sat_grads* g, const echr_dropout* drop, void* stream) {
    return sat_bwd(a, g, drop, nullptr, "sat_bwd", stream);
}
extern "C" int echr_sat_bwd_batch(const echr_sat_args* a, const echr_sat_grads* g, const echr_dropout* drop, const echr_batch_ext* x, void* stream) {
    ECHR_REQUIRE(x, "sat_bwd_batch: null batch extension");
    return sat_bwd(a, g, drop, x, "sat_bwd_batch", stream);
}
