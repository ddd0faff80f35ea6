// hmm_dense.hip -- forward-backward of the HMM with a full K x K transition matrix over a mixture's components
// (abny_hmm_dense_forward_backward) and the expected transition counts of its Baum-Welch step.
// abnet3_amd/hmm.py states the definition; DESIGN.md section 3.4c6 the shape.  The launch shape, the score block's logN half,
// the matrix in LDS and the launcher are hmm_dense.h's, described there; workspace geometry and checks are utt_chain.h's.
//
// hmm_fb_kernel's twin (hmm.hip): the slab of a block is rewritten in place as bt = exp(logN - m_t) (the sticky kernel's
// bits), then one sequential step per frame and sweep.  `post` is the store of ahat between the sweeps; c_t per frame goes
// to the workspace.  What is new:
//   * the transition matrix is zero past K.  The forward step reads a column slice trans[j0 .. j0 + SW - 1][k] with the
//     lanes over k: consecutive dwords.  The backward step reads a row slice trans[j][k0 .. k0 + SW - 1] with the lanes over
//     j: KC + 1 dwords apart, 32 different banks for the 32 lanes of a ds_read_b32 group.
//   * own is k forward and j backward; the NS partial sums are added slice 0 first.  c_t is ONE sum reduction (DPP inside
//     the wave, one LDS exchange, w0 + w1 + w2 + w3).
//   * G[j][k] += ahat_p[j] e_t[k] is a rank-one update per transition, off the chain: thread t owns the SW cells
//     (own, sl SW + c) in registers (64 at KC = 128), adds over a block of at most 128 frames in fp32 and then into its own
//     cells of the workgroup's float64 slab in the workspace (cell c of thread t at [c][t]: a coalesced row per c; behind
//     the KC^2 cells the KC of `first`).  Every cell is read and written by the one thread that owns it.  A second small
//     launch (hmm_dense_stats_kernel) adds the workgroups' slabs in workgroup order and applies xi = trans o G once.
// No floating-point atomic; nothing of an utterance's results depends on the grid or on its neighbours, and the statistics
// depend on the grid only through min(n_utt, 256).
#include "fixed_sum.h"
#include "hmm_dense.h"
#include "../../include/abnet3_hip_next.h"

namespace abn {

constexpr int64_t HD_FRAME_BYTES = sizeof(float);         // c_t per frame
constexpr int64_t hd_stats_bytes(int kc) { return (int64_t)sizeof(double) * (kc * kc + kc); }      // G cells, then `first`

struct HmmDenseP {
    GmmP g;                                 // x, shift, A, B, c = c0, T, K, D, tiles_k: a kernel argument, as in hmm.hip
    const float* init; const float* trans;
    const int64_t* off; const int* len;
    int n_utt, mode, want_stats;
    float* post; double* loglik; int* n_good;
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, cap;                            // slab row stride (floats), frames the region holds
};

// The block of frames m0 .. m0 + nf - 1: hd_logn_block, then the slab rewritten as bt and m_t (hmm_block_scores of hmm.hip
// with every component live: the same tile, the same max, the same expf).  Ends behind a barrier.
__device__ __forceinline__ void hd_block_scores(const HmmDenseP& p, int m0, int nf, float* smem, float* slab, int* bad_s,
                                                float* mt_s)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ks = p.ks;
    const GmmP& gp = p.g;
    hd_logn_block(gp, m0, nf, smem, slab, ks, bad_s);
    for (int f = wave; f < nf; f += 4) {                              // wave w takes frames w, w + 4, ...: lanes over k
        float* const row = slab + (int64_t)f * ks;
        float m = -INFINITY;
        for (int k = lane; k < gp.K; k += 64) m = fmaxf(m, row[k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        for (int k = lane; k < gp.K; k += 64) row[k] = expf(row[k] - m);
        if (lane == 0) mt_s[f] = m;
    }
    __syncthreads();
}

template <int KC>
__global__ __launch_bounds__(256) void hmm_dense_kernel(HmmDenseP p)
{
    constexpr int NS = 256 / KC, SW = KC / NS, TS = KC + 1;
    static_assert(NS * SW == KC && NS * KC == 256, "256 threads cover KC x KC in slices of SW");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int bad_s[GM_B];
    __shared__ float mt_s[GM_B], c_s[GM_B];
    __shared__ float red_s[4];
    __shared__ double red_d[256];
    __shared__ float part_s[256];                                     // [slice][own]
    __shared__ float vec_s[2][KC];                                    // forward: ahat in [0]; backward: e, by parity
    __shared__ float ah_s[KC];                                        // backward: the current frame's ahat

    float* const tr_s = smem + 4 * GmTile::floats;                    // [KC][TS], behind the operand tiles
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int own = t % KC, sl = t / KC;
    const int K = p.g.K, ks = p.ks;
    const bool owner = t < K;                                         // component t's chain values live in this thread
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = reinterpret_cast<float*>(base);
    double* const gs = reinterpret_cast<double*>(base + (int64_t)sizeof(float) * GM_B * ks);
    float* const cw = reinterpret_cast<float*>(base + (int64_t)sizeof(float) * GM_B * ks + hd_stats_bytes(KC));
    const bool want_stats = p.want_stats != 0;

    hd_load_matrix<KC>(tr_s, p.trans, K, 0.0f, false);
    if (want_stats) {                                                 // this thread's own cells
#pragma unroll
        for (int c = 0; c < SW; ++c) gs[c * 256 + t] = 0.0;
        if (t < KC) gs[KC * KC + t] = 0.0;
    }
    const float pi = owner ? p.init[t] : 0.0f;
    if (t < KC) { vec_s[0][t] = 0.0f; vec_s[1][t] = 0.0f; ah_s[t] = 0.0f; }
    __syncthreads();

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (hd_out_of_range(o, L, p.g.T, p.cap)) {                    // (uniform) nothing of this utterance is touched
            if (t == 0) {
                p.loglik[u] = NAN;
                p.n_good[u] = -1;
            }
            continue;
        }
        float* const post = p.post + o * K;
        float bh = 0.0f;                                              // backward: bhat[t] of the current frame
        bool started = false, have_e = false;
        int ngood = 0, remaining = 0, par = 0;
        double ll = 0.0;

        // Steps 0 .. nblk - 1: the forward sweep over the blocks; steps nblk .. 2 nblk - 1 (mode 0): the backward sweep,
        // last block first.  (One loop, so that the score phase is in the kernel once.)
        const int nblk = (L + GM_B - 1) / GM_B;
        const int nstep = p.mode == 0 ? 2 * nblk : nblk;
        for (int step = 0; step < nstep; ++step) {
            const bool fwd = step < nblk;
            if (step == nblk) {                                       // (uniform) the turn: bhat = 1 at the last good frame
                if (ngood < 1) break;
                remaining = ngood;
                bh = 1.0f;
            }
            const int f0 = (fwd ? step : 2 * nblk - 1 - step) * GM_B;
            const int nf = min(GM_B, L - f0);
            if (!fwd && t < nf) c_s[t] = cw[f0 + t];                  // (thread 0's stores of the forward sweep, barriers behind)
            hd_block_scores(p, (int)o + f0, nf, smem, slab, bad_s, mt_s);

            if (fwd) {
                float bn = owner ? slab[t] : 0.0f;
                for (int f = 0; f < nf; ++f) {
                    const float b = bn;
                    if (f + 1 < nf) bn = owner ? slab[(int64_t)(f + 1) * ks + t] : 0.0f;
                    float* const prow = post + (int64_t)(f0 + f) * K;
                    if (bad_s[f]) {                                   // (uniform) the chain passes over it
                        if (owner) prow[t] = 0.0f;
                        continue;
                    }
                    float pred = pi;
                    if (started) {                                    // (uniform) pred[own] = sum_j ahat[j] trans[j][own]
                        const float* const trc = tr_s + (sl * SW) * TS + own;
                        const float* const av = vec_s[0] + sl * SW;
                        float acc = 0.0f;
#pragma unroll
                        for (int c = 0; c < SW; ++c) acc = fmaf(av[c], trc[c * TS], acc);
                        part_s[t] = acc;
                        __syncthreads();
                        pred = part_s[own];
#pragma unroll
                        for (int s = 1; s < NS; ++s) pred += part_s[s * KC + own];
                    }
                    const float uu = owner ? b * pred : 0.0f;
                    const float s = fixed_wave_sum(uu);
                    if (lane == 0) red_s[wave] = s;
                    __syncthreads();
                    const float c = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
                    const float a = uu * (1.0f / c);
                    if (owner) {
                        vec_s[0][t] = a;
                        prow[t] = a;
                    }
                    if (t == 0) { c_s[f] = c; cw[f0 + f] = c; }
                    __syncthreads();                                  // ahat is in vec_s; red_s and part_s are free again
                    started = true;
                    ++ngood;
                }
                __syncthreads();                                      // c_s is complete; the slab's readers are done
                double v = 0.0;
                if (t < nf && !bad_s[t]) v = log((double)c_s[t]) + (double)mt_s[t];
                ll += fixed_block_sum(v, red_d);
            } else {
                float G[SW];
#pragma unroll
                for (int c = 0; c < SW; ++c) G[c] = 0.0f;
                float bn = owner ? slab[(int64_t)(nf - 1) * ks + t] : 0.0f;
                float an = owner ? post[(int64_t)(f0 + nf - 1) * K + t] : 0.0f;
                for (int f = nf - 1; f >= 0; --f) {
                    const float b = bn, ah = an;
                    if (f > 0) {
                        bn = owner ? slab[(int64_t)(f - 1) * ks + t] : 0.0f;
                        an = owner ? post[(int64_t)(f0 + f - 1) * K + t] : 0.0f;
                    }
                    if (bad_s[f]) continue;                           // (uniform)
                    const float gam = ah * bh;
                    if (owner) post[(int64_t)(f0 + f) * K + t] = gam;
                    const bool first = --remaining == 0;              // (uniform) the first good frame has no predecessor
                    if (have_e || !first) {                           // (uniform)
                        if (t < KC) {
                            ah_s[t] = ah;
                            if (!first) vec_s[par][t] = b * bh * (1.0f / c_s[f]);
                        }
                        __syncthreads();
                        if (have_e && want_stats) {                   // the transition into the later frame: its e is in [par ^ 1]
                            const float aj = ah_s[own];
                            const float* const ev = vec_s[par ^ 1] + sl * SW;
#pragma unroll
                            for (int c = 0; c < SW; ++c) G[c] = fmaf(aj, ev[c], G[c]);
                        }
                    }
                    if (first) {
                        if (want_stats && owner) gs[KC * KC + t] += (double)gam;
                        break;
                    }
                    {                                                 // bhat[own] <- sum_k trans[own][k] e[k]
                        const float* const trr = tr_s + own * TS + sl * SW;
                        const float* const ev = vec_s[par] + sl * SW;
                        float acc = 0.0f;
#pragma unroll
                        for (int c = 0; c < SW; ++c) acc = fmaf(trr[c], ev[c], acc);
                        part_s[t] = acc;
                        __syncthreads();
                        float nb = part_s[own];
#pragma unroll
                        for (int s = 1; s < NS; ++s) nb += part_s[s * KC + own];
                        bh = nb;                                      // (every slice's thread holds it; the owners use it)
                    }
                    have_e = true;
                    par ^= 1;
                }
                if (want_stats) {
                    // tb is t behind an empty asm: the SW addresses of these cells are formed here, not kept in registers
                    // across the launch as loop invariants (the compiler did that, and spilled them to scratch)
                    int tb = t;
                    asm volatile("" : "+v"(tb));
                    double* const gc = gs + tb;
#pragma unroll
                    for (int c = 0; c < SW; ++c) gc[c * 256] += (double)G[c];
                }
                __syncthreads();                                      // before the next block's scores replace these
                if (remaining == 0) break;                            // (uniform)
            }
        }
        if (t == 0) {
            p.loglik[u] = ll;
            p.n_good[u] = ngood;
        }
        __syncthreads();
    }
}

// stats [K + 1][K] float64 from the workgroups' slabs, in workgroup order: rows 0 .. K - 1 xi = trans o G, row K `first`.
__global__ __launch_bounds__(256) void hmm_dense_stats_kernel(const char* __restrict__ ws, int64_t per_wg, int64_t slab_bytes,
                                                              int grid, int K, int kc, const float* __restrict__ trans,
                                                              double* __restrict__ stats)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= (K + 1) * K) return;
    const int r = i / K, k = i % K;
    const int sw = kc * kc / 256;
    const int cell = r < K ? (k % sw) * 256 + (k / sw) * kc + r : kc * kc + k;
    double a = 0.0;
    for (int g = 0; g < grid; ++g) a += reinterpret_cast<const double*>(ws + (int64_t)g * per_wg + slab_bytes)[cell];
    stats[i] = r < K ? (double)trans[i] * a : a;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abny_hmm_dense_max_k(void) { return HD_MAX_K; }

extern "C" int64_t abny_hmm_dense_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D)
{
    return chain_ws_bytes("abny_hmm_dense_ws_bytes", n_utt, max_len, K, D, HD_LIMITS, HD_FRAME_BYTES,
                          K >= 1 && K <= HD_MAX_K ? hd_stats_bytes(hd_kc_for(K)) : 0);
}

extern "C" int abny_hmm_dense_forward_backward(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len,
                                               int64_t n_utt, const float* shift, const float* A, const float* B,
                                               const float* c0, const float* init, const float* trans, int64_t K, int mode,
                                               float* post, double* loglik, int32_t* n_good, double* stats, void* ws,
                                               int64_t ws_bytes, void* stream)
{
    const char* what = "abny_hmm_dense_forward_backward";
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - GM_B, "%s: T = %lld out of range", what, (long long)T);
    int rc = chain_check_sizes(what, n_utt, K, D, HD_LIMITS);
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && off && len && shift && A && B && c0 && init && trans && post && loglik && n_good, "%s: null pointer", what);
    ABN_REQUIRE(mode == 0 || mode == 1, "%s: mode = %d, 0 (smoothed) or 1 (filtered)", what, mode);
    const int kc = hd_kc_for(K);
    const ChainWs hw = chain_ws(n_utt, 0, K, HD_FRAME_BYTES, hd_stats_bytes(kc));
    ChainRegion a;
    rc = chain_region(what, "abny_hmm_dense_ws_bytes", ws, ws_bytes, hw, &a);
    if (rc != ABN_OK) return rc;
    HmmDenseP p;
    p.g = hmm_score_params(x, T, D, shift, A, B, c0, K);      // (K <= 128: one tile of components)
    p.init = init; p.trans = trans; p.off = off; p.len = len; p.n_utt = (int)n_utt;
    p.mode = mode; p.want_stats = stats != nullptr;
    p.post = post; p.loglik = loglik; p.n_good = n_good;
    p.ws = a.ws; p.per_wg = a.per_wg;
    p.ks = a.ks; p.cap = a.cap;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hd_for_kc(kc, [&](auto c) {
        constexpr int KC = decltype(c)::value;
        hd_launch<hmm_dense_kernel<KC>, KC>(p, hw.grid, st);
    });
    ABN_CHECK_LAUNCH(what);
    if (stats) {
        const int cells = (int)((K + 1) * K);
        hipLaunchKernelGGL(hmm_dense_stats_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a.ws, a.per_wg,
                           hw.slab_bytes, hw.grid, (int)K, kc, trans, stats);
        ABN_CHECK_LAUNCH("abny_hmm_dense_forward_backward (statistics)");
    }
    return ABN_OK;
}
