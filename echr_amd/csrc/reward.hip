// CIDEr-D over token ids (echr_ciderd_score): the reward of self-critical training and the package's validation
// metric.  One workgroup per candidate row; the row's n-gram keys and tf-idf weights live in LDS and the row's references are streamed
// through a second set of the same arrays.
//
// Sequence of a row under seq_length L: the l tokens before its first 0 among columns < T (l = T when there is none), then one end token 0
// iff l < L.  An n-gram's key is the exact packing sum (tok_i + 1) << 16 i, i < n <= 4: the order is the number of non-zero fields, so the
// keys of different orders never collide and one sorted table holds them all.
//
// Arithmetic: fp64 throughout, in one fixed order -- a thread owns an n-gram (tf by comparing keys, idf by binary search in the table,
// the matching reference weight by scanning the reference's n-grams of its order), and thread n - 1 sums order n serially in n-gram
// order.  No atomics, no cross-workgroup traffic: a row's score does not depend on which rows share its launch.
#include "echr_common.h"
#include "echr_internal.h"

namespace echr {

constexpr int CD_MAX_L = 63;                        // sequence tokens, end token included (l = L carries none)
constexpr int CD_MAX_G = 4 * CD_MAX_L - 6;          // 63 + 62 + 61 + 60 n-grams
constexpr int CD_THREADS = 256;
constexpr int CD_MAX_TOK = 65534;                   // tok + 1 fits a 16-bit field

struct CdGrams {                                    // one sequence's n-grams (LDS)
    int tok[CD_MAX_L + 1];
    uint64_t key[CD_MAX_G];
    double w[CD_MAX_G];                             // tf * idf at an n-gram's first occurrence, 0 at a repeat
    unsigned char first[CD_MAX_G];
    double norm[4];
    int len;
};

__device__ __forceinline__ int cd_count(int len, int n) { return max(0, len - n + 1); }             // n-grams of order n
__device__ __forceinline__ int cd_start(int len, int n) {                                           // index of the first one
    int s = 0;
    for (int m = 1; m < n; ++m) s += cd_count(len, m);
    return s;
}

// keys, first-occurrence flags, weights and per-order norms of s.tok[0 .. s.len) -- every thread of the workgroup calls it
__device__ void cd_weights(CdGrams& s, const uint64_t* __restrict__ keys, const double* __restrict__ idf, int n_keys,
                           double idf_unseen, int tid) {
    const int len = s.len;
    const int G = cd_start(len, 5);
    int n = 1;
    while (n < 4 && tid >= cd_start(len, n + 1)) ++n;
    const int g0 = cd_start(len, n), gc = cd_count(len, n);
    uint64_t key = 0;
    if (tid < G) {
        const int pos = tid - g0;
        for (int i = 0; i < n; ++i) key |= (uint64_t)(s.tok[pos + i] + 1) << (16 * i);
        s.key[tid] = key;
    }
    __syncthreads();
    if (tid < G) {
        int tf = 0;
        bool first = true;
        for (int j = g0; j < g0 + gc; ++j) {
            const bool eq = s.key[j] == key;
            tf += eq;
            first = first && !(eq && j < tid);
        }
        double w = 0.0;
        if (first) {
            int lo = 0, hi = n_keys;
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                if (keys[mid] < key) lo = mid + 1; else hi = mid;
            }
            const double f = (lo < n_keys && keys[lo] == key) ? idf[lo] : idf_unseen;
            w = (double)tf * f;
        }
        s.w[tid] = w;
        s.first[tid] = first;
    }
    __syncthreads();
    if (tid < 4) {
        const int a = cd_start(len, tid + 1), c = cd_count(len, tid + 1);
        double q = 0.0;
        for (int j = a; j < a + c; ++j) q += s.w[j] * s.w[j];
        s.norm[tid] = sqrt(q);
    }
    __syncthreads();
}

__device__ __forceinline__ int cd_token(long long v) { return (int)(v < 0 ? 0 : (v > CD_MAX_TOK ? CD_MAX_TOK : v)); }

__global__ __launch_bounds__(CD_THREADS) void ciderd_kernel(const echr_ciderd_args a) {
    __shared__ CdGrams H, R;
    __shared__ double s_c[CD_MAX_G], s_acc[4];
    __shared__ int s_T;
    const int row = blockIdx.x, tid = threadIdx.x, L = a.L;
    if (tid == 0) {
        int T = a.T;
        if (a.counts) {          // functional._stop_step: the first t in 1..L with nobody unfinished gives t - 1
            T = L;
            for (int t = 1; t <= L; ++t)
                if (a.counts[t] == 0) { T = t - 1; break; }
        }
        s_T = min(max(T, 0), L);
    }
    __syncthreads();
    const int T = s_T;
    if (tid < 64) {              // T <= 63: wave 0 holds the whole row
        long long v = 1;
        if (tid < T) {
            const int64_t at = (int64_t)row * a.ld + (int64_t)tid * a.cs;
            v = a.cand_i32 ? (long long)((const int32_t*)a.cand)[at] : (long long)((const int64_t*)a.cand)[at];
            H.tok[tid] = cd_token(v);
        }
        const unsigned long long zeros = __ballot(tid < T && v == 0);
        if (tid == 0) {
            const int l = zeros ? __ffsll((long long)zeros) - 1 : T;
            if (l < L) H.tok[l] = 0;
            H.len = l + (l < L ? 1 : 0);
        }
    }
    __syncthreads();
    cd_weights(H, a.keys, a.idf, a.n_keys, a.idf_unseen, tid);
    const int hl = H.len, GH = cd_start(hl, 5);
    int n = 1;
    while (n < 4 && tid >= cd_start(hl, n + 1)) ++n;
    const int r0 = min(max(a.ref_offset[row], 0), a.R_tot), r1 = min(max(a.ref_offset[row + 1], r0), a.R_tot);
    double acc = 0.0;            // thread n - 1: sum over the references of val_n
    for (int r = r0; r < r1; ++r) {
        const int rl = min(max(a.ref_len[r], 1), L);
        if (tid < rl) R.tok[tid] = cd_token(a.refs[(int64_t)r * L + tid]);
        if (tid == 0) R.len = rl;
        __syncthreads();
        cd_weights(R, a.keys, a.idf, a.n_keys, a.idf_unseen, tid);
        if (tid < GH) {
            double c = 0.0;
            if (H.first[tid]) {
                const uint64_t key = H.key[tid];
                const int b = cd_start(rl, n), e = b + cd_count(rl, n);
                double wr = 0.0;
                for (int j = b; j < e; ++j)
                    if (R.first[j] && R.key[j] == key) wr = R.w[j];
                c = fmin(H.w[tid], wr) * wr;
            }
            s_c[tid] = c;
        }
        __syncthreads();
        if (tid < 4) {
            const int b = cd_start(hl, tid + 1), e = b + cd_count(hl, tid + 1);
            double v = 0.0;
            for (int j = b; j < e; ++j) v += s_c[j];
            const double nh = H.norm[tid], nr = R.norm[tid];
            if (nh != 0.0 && nr != 0.0) v /= nh * nr;
            const double d = (double)(hl - rl);
            acc += v * exp(-(d * d) / 72.0);          // sigma = 6
        }
        __syncthreads();
    }
    if (tid < 4) s_acc[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        const int nr = r1 - r0;
        double sc = nr > 0 ? 10.0 * ((((s_acc[0] + s_acc[1]) + s_acc[2]) + s_acc[3]) / 4.0) / (double)nr : 0.0;
        if (a.base) sc = (double)a.weight * (sc - (double)a.base[row]);
        a.out[row] = (float)sc;
    }
}

}  // namespace echr

using namespace echr;

extern "C" int echr_ciderd_score(const echr_ciderd_args* a, void* stream) {
    ECHR_REQUIRE(a != nullptr, "echr_ciderd_score: null arguments");
    ECHR_REQUIRE(a->N >= 0, "echr_ciderd_score: N = %d", a->N);
    ECHR_REQUIRE(a->L >= 1 && a->L <= CD_MAX_L, "echr_ciderd_score: seq_length %d outside [1, %d]", a->L, CD_MAX_L);
    ECHR_REQUIRE(a->counts != nullptr || (a->T >= 0 && a->T <= a->L), "echr_ciderd_score: width %d outside [0, seq_length = %d]", a->T, a->L);
    ECHR_REQUIRE(a->n_keys >= 0 && (a->n_keys == 0 || (a->keys && a->idf)), "echr_ciderd_score: a table of %d keys needs keys and idf", a->n_keys);
    ECHR_REQUIRE(a->R_tot >= 0 && (a->R_tot == 0 || (a->refs && a->ref_len)), "echr_ciderd_score: %d references need refs and ref_len", a->R_tot);
    if (a->N == 0) return 0;
    ECHR_REQUIRE(a->cand && a->ref_offset && a->out, "echr_ciderd_score: cand, ref_offset and out are required");
    hipLaunchKernelGGL(ciderd_kernel, dim3(a->N), dim3(CD_THREADS), 0, (hipStream_t)stream, *a);
    return check_launch("ciderd_score");
}
