// Frame-level contexts 'CH' and 'CC+CH' (CaptionGenerator.py:140-167, change_context_dim :56-84): the attended clip rows are the proposal
// encoder's states tap_feats, alone ('CH', D = Ht) or behind the C3D rows ('CC+CH', D = Dc + Ht).  The forward pass is the decoder's own
// (echr_dec_args.c3d is just a row source of runtime width D); what this file adds is the gradient with respect to the attended rows, the
// third path by which the caption loss reaches the proposal encoder, and the row source of 'CC+CH':
//
//   d rows[start_n + a, c] += sum_t WT[t,n,a] . d att[t,n,c]  +  (d P_all . W_c2a)[start_n + a, c]      (a < len_n, c in [col0, col0 + ncols))
//   d att[t,n,:] = d gates1[t,n,:] . W_ih1[:, E + col0 : E + col0 + ncols]
//
// d gates1 (DG[1]) and d P_all (DPALL, already the per-row sum over the events) are what echr_decoder_bwd leaves in its backward workspace.
#include <cstdio>

#include "echr_common.h"
#include "echr_internal.h"

#define RC(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

namespace echr {

static inline long up64(long n) { return (n + 63) / 64 * 64; }

// rows[r, :] = [c3d[r, :Dc] | tap[r, :Ht]]   (one workgroup per row)
__global__ __launch_bounds__(256) void clip_rows_kernel(const float* __restrict__ c3d, const float* __restrict__ tap, float* __restrict__ rows,
                                                        int Dc, int Ht) {
    const long r = blockIdx.x;
    const int D = Dc + Ht;
    for (int j = threadIdx.x; j < D; j += 256) rows[r * D + j] = j < Dc ? c3d[r * Dc + j] : tap[r * Ht + (j - Dc)];
}

// live[i] = 1 for the listed time-major rows t*N + n (echr_train_step's active rows), 0 elsewhere (the caller zero-fills)
__global__ __launch_bounds__(256) void live_rows_kernel(const int* __restrict__ act, int n_act, int* __restrict__ live) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_act) live[act[i]] = 1;
}

// Context term.  One workgroup per (event n, chunk of RG_SLOTS slots): the event's d att rows [S, nc] are read once per chunk and weighted by
// every slot's attention weight.  Slots at or beyond len_n are skipped: their weight is zero but their row index belongs to other events.
// Rows t*N + n that are not live (behind a caption's last masked position on the compacted one-call path) count as zero: skipped, never read
// as values.  mode 0: plain read-modify-write of out (no two events share a row); 1: atomic adds; 2: slab[(n*A + a)*nc + c] (fixed order).
constexpr int RG_SLOTS = 8;
constexpr int RG_LIST_MAX_S = 4096;          // row_grad_scatter_list_kernel: 16 KB of LDS flags at most
__global__ __launch_bounds__(256) void row_grad_scatter_kernel(const float* __restrict__ WT, const float* __restrict__ DATT, const int* __restrict__ live,
                                                               const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                               float* __restrict__ out, long ld, float* __restrict__ slab, int S, int N, int A, int nc, int mode) {
    const int n = blockIdx.y, a0 = blockIdx.x * RG_SLOTS;
    const int len = ev_len[n];
    if (a0 >= len) return;
    const int na = min(RG_SLOTS, len - a0);
    const long start = ev_start[n];
    for (int c = threadIdx.x; c < nc; c += 256) {
        float s[RG_SLOTS];
#pragma unroll
        for (int k = 0; k < RG_SLOTS; ++k) s[k] = 0.f;
        for (int t = 0; t < S; ++t) {
            const long rn = (long)t * N + n;
            if (live && !live[rn]) continue;
            const float v = DATT[rn * nc + c];
            const float* w = WT + rn * A + a0;
#pragma unroll
            for (int k = 0; k < RG_SLOTS; ++k)
                if (k < na) s[k] += w[k] * v;
        }
#pragma unroll
        for (int k = 0; k < RG_SLOTS; ++k) {
            if (k >= na) break;
            if (mode == 2) slab[((long)n * A + a0 + k) * nc + c] = s[k];
            else if (mode == 1) atomicAdd(out + (start + a0 + k) * ld + c, s[k]);
            else out[(start + a0 + k) * ld + c] += s[k];
        }
    }
}

// The same term with the compacted row list read directly (echr_train_step_batch_clip): the workgroup of an (event, chunk) first marks its event's
// live steps in LDS -- lv[t] = 1 for every listed row t*N + n' with n' == n -- then runs the loop above in the same t order, so the sums are those
// of row_grad_scatter_kernel bit for bit.  No [S*N] flag array, no fill and no marking launch in front of it.  act == nullptr: every row is live.
// Dynamic LDS: S ints.  Dead rows are skipped, never read as values.
__global__ __launch_bounds__(256) void row_grad_scatter_list_kernel(const float* __restrict__ WT, const float* __restrict__ DATT, const int* __restrict__ act,
                                                                    int n_act, const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                                    float* __restrict__ out, long ld, float* __restrict__ slab, int S, int N, int A, int nc,
                                                                    int mode) {
    extern __shared__ int lv[];
    const int n = blockIdx.y, a0 = blockIdx.x * RG_SLOTS;
    const int len = ev_len[n];
    if (a0 >= len) return;          // (uniform over the workgroup: in front of every barrier)
    const int na = min(RG_SLOTS, len - a0);
    const long start = ev_start[n];
    if (act) {
        for (int t = threadIdx.x; t < S; t += 256) lv[t] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n_act; i += 256) {
            const int r = act[i], t = r / N;
            if (r >= 0 && t < S && r - t * N == n) lv[t] = 1;
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < nc; c += 256) {
        float s[RG_SLOTS];
#pragma unroll
        for (int k = 0; k < RG_SLOTS; ++k) s[k] = 0.f;
        for (int t = 0; t < S; ++t) {
            if (act && !lv[t]) continue;
            const long rn = (long)t * N + n;
            const float v = DATT[rn * nc + c];
            const float* w = WT + rn * A + a0;
#pragma unroll
            for (int k = 0; k < RG_SLOTS; ++k)
                if (k < na) s[k] += w[k] * v;
        }
#pragma unroll
        for (int k = 0; k < RG_SLOTS; ++k) {
            if (k >= na) break;
            if (mode == 2) slab[((long)n * A + a0 + k) * nc + c] = s[k];
            else if (mode == 1) atomicAdd(out + (start + a0 + k) * ld + c, s[k]);
            else out[(start + a0 + k) * ld + c] += s[k];
        }
    }
}

// fixed-order fold of the per-(event, slot) slabs: row r gathers the slots that address it in event order (as dpall_fold_kernel does for d P_all)
__global__ __launch_bounds__(256) void row_grad_fold_kernel(const float* __restrict__ slab, const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                            float* __restrict__ out, long ld, int N, int A, int nc) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < nc; c += 256) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) {
            const int a = r - ev_start[n];
            if (a >= 0 && a < ev_len[n]) s += slab[((long)n * A + a) * nc + c];
        }
        out[(long)r * ld + c] += s;
    }
}

struct RowGradWs { float* DATT; int* LIVE; long total; };
static RowGradWs carve_row_grad(const echr_dec_args* a, int ncols, float* base) {
    RowGradWs w;
    const long SN = (long)a->S * a->N;
    w.DATT = base;
    w.LIVE = base ? reinterpret_cast<int*>(base + up64(SN * ncols)) : nullptr;
    w.total = up64(SN * ncols) + up64(SN);
    return w;
}

int clip_rows(const float* c3d, int Dc, const float* tap, int Ht, float* rows, int Tv, hipStream_t st) {
    ECHR_REQUIRE(c3d && tap && rows && Dc > 0 && Ht > 0 && Tv > 0, "clip_rows: bad arguments");
    hipLaunchKernelGGL(clip_rows_kernel, dim3(Tv), dim3(256), 0, st, c3d, tap, rows, Dc, Ht);
    return check_launch("clip_rows");
}

int row_grad(const echr_dec_args* a, const echr_dec_grads* g, const echr_row_grad_args* r, hipStream_t st, bool list_form) {
    ECHR_REQUIRE(a && g && r, "decoder_row_grad: null arguments");
    ECHR_REQUIRE(a->ws && g->ws_bwd && r->out && r->ws, "decoder_row_grad: missing buffers");
    ECHR_REQUIRE(r->ncols > 0 && r->col0 >= 0 && r->col0 + r->ncols <= a->D && r->ld >= r->ncols,
                 "decoder_row_grad: columns [%d, %d) do not lie in the %d-wide row source (ld %lld)", r->col0, r->col0 + r->ncols, a->D, (long long)r->ld);
    ECHR_REQUIRE(a->N > 0 && a->A > 0 && a->Tv > 0 && a->S > 0, "decoder_row_grad: bad N/A/Tv/S");
    // d P_all comes out of the backward pass's attention stage, which may still run on a helper stream (asynchronous tail): order it first
    RC(join_tail(st));
    const int N = a->N, S = a->S, A = a->A, H = a->H, E = a->E, Ha = a->Ha, D = a->D, nc = r->ncols;
    const long SN = (long)S * N;
    const int cin1 = E + D;
    const float* DG1 = nullptr;
    const float* DPALL = nullptr;
    decoder_bwd_views(a, g, &DG1, &DPALL);
    const float* WT = decoder_fwd_wt(a);
    RowGradWs w = carve_row_grad(a, nc, r->ws);
    // context term: d att for the wanted columns over all S*N rows (one product), then the weighted scatter onto the rows
    echr_gemm_desc d = desc_nn(DG1, 4 * H, a->w_ih[1] + E + r->col0, cin1, w.DATT, nc, (int)SN, nc, 4 * H);
    RC(gemm(d, st));
    const int* live = nullptr;
    const bool compact = g->active_rows && g->n_active > 0;
    // (the list form keeps S flags in LDS: a step count beyond that budget -- never a caption's -- takes the flag form)
    list_form = list_form && config().row_grad_list && S <= RG_LIST_MAX_S;
    if (compact && !list_form) {
        RC(fill_zero(reinterpret_cast<float*>(w.LIVE), SN, st));
        hipLaunchKernelGGL(live_rows_kernel, dim3((g->n_active + 255) / 256), dim3(256), 0, st, g->active_rows, g->n_active, w.LIVE);
        RC(check_launch("row_grad_live"));
        live = w.LIVE;
    }
    const bool fixed = det_mode() && !a->rows_disjoint;
    float* slab = nullptr;
    if (fixed) { slab = det_scratch(DET_ROWG, (size_t)N * A * nc); if (!slab) return -12; }
    const int mode = fixed ? 2 : (a->rows_disjoint ? 0 : 1);
    if (list_form)
        hipLaunchKernelGGL(row_grad_scatter_list_kernel, dim3((A + RG_SLOTS - 1) / RG_SLOTS, N), dim3(256), sizeof(int) * (size_t)S, st, WT, w.DATT,
                           compact ? g->active_rows : nullptr, compact ? g->n_active : 0, a->ev_start, a->ev_len, r->out, (long)r->ld, slab, S, N, A, nc, mode);
    else
    hipLaunchKernelGGL(row_grad_scatter_kernel, dim3((A + RG_SLOTS - 1) / RG_SLOTS, N), dim3(256), 0, st, WT, w.DATT, live, a->ev_start, a->ev_len,
                       r->out, (long)r->ld, slab, S, N, A, nc, mode);
    RC(check_launch("row_grad_scatter"));
    if (fixed) {
        hipLaunchKernelGGL(row_grad_fold_kernel, dim3(a->Tv), dim3(256), 0, st, slab, a->ev_start, a->ev_len, r->out, (long)r->ld, N, A, nc);
        RC(check_launch("row_grad_fold"));
    }
    // projection term: out[Tv, nc] += d P_all [Tv, Ha] . W_c2a[:, col0 : col0 + nc]  (one k slice: a plain read-modify-write, fixed order)
    d = desc_nn(DPALL, Ha, a->w_c2a + r->col0, D, r->out, r->ld, a->Tv, nc, Ha);
    d.beta = 1.f; d.split_k = 1;
    return gemm(d, st);
}

}  // namespace echr

using namespace echr;

extern "C" int64_t echr_decoder_row_grad_ws_floats(const echr_dec_args* a, int32_t ncols) {
    return (a && ncols > 0) ? carve_row_grad(a, ncols, nullptr).total : -1;
}

extern "C" int echr_decoder_row_grad(const echr_dec_args* a, const echr_dec_grads* g, const echr_row_grad_args* r, void* stream) {
    RC(check_dims_public(a, "decoder_row_grad"));
    return row_grad(a, g, r, (hipStream_t)stream);
}

extern "C" int echr_clip_rows(const float* c3d, int32_t Dc, const float* tap, int32_t Ht, float* rows, int32_t Tv, void* stream) {
    return clip_rows(c3d, Dc, tap, Ht, rows, Tv, (hipStream_t)stream);
}
