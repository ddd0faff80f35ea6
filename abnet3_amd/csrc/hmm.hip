// hmm.hip -- forward-backward of the sticky HMM over a mixture's components (abn_hmm_forward_backward, and with the
// per-component stays abn_hmm_forward_backward_stats), the statistics of its Baum-Welch step (abn_hmm_accumulate) and
// its max-product path (abn_hmm_viterbi, above hmm_viterbi_kernel).
// abnet3_amd/hmm.py states the definition; DESIGN.md section 3.4c2 the shape.  The host side of the three per-utterance
// kernels (workspace geometry, checks, NQ dispatch) is utt_chain.h's, shared with kmeans.hip.
//
// The sum-product twin of km_viterbi_kernel (kmeans.hip): one launch for the corpus, persistent workgroups that loop
// over the utterances, a slab of 128 frames x K emission scores from the mixture's own fp32 MFMA tile (gmm_tile.h, with
// c0 = c without the log weight as the third table), then one sequential step per frame.  Per block of 128 frames:
//   * parallel: the score tiles into the slab; m_t = max over {k : w[k] > 0} (a wave per frame, lanes over k; a max has
//     no rounding, so its order does not matter); the slab is rewritten in place as bt = exp(logN - m_t), 0 where
//     w[k] = 0 (such a component's pred is exactly 0 in every frame, so its bt is never a factor of anything);
//   * forward, sequential: component k = 256 q + thread, ahat in registers; u = bt (rho ahat + (1 - rho) w), c_t = sum_k u
//     by ONE sum reduction (q ascending in the thread, DPP inside the wave, one LDS exchange across the four waves,
//     w0 + w1 + w2 + w3), ahat = u / c_t written straight into `post`: the output buffer is the store of ahat;
//   * parallel: sum over the block's good frames of log c_t + m_t in float64, a fixed tree.
// Mode 0 then walks the blocks last to first: the block's bt slab is recomputed (the same bits), c_t comes back from the
// workspace, ahat_t from `post` -- every thread reads back exactly the elements it wrote itself --, and
//   gamma_t = ahat_t bhat,  e = bt bhat / c_t,  bhat <- rho e + (1 - rho) sum_k w e
// with again one sum reduction per frame.  The expected stays sum_k rho ahat_p e_t are off the chain: a float64
// accumulator per thread, summed over the workgroup in a fixed tree at the utterance's end.
// The workspace of a workgroup: the slab and c_t per frame.  There is no T x K array beyond the output, no
// floating-point atomic, and nothing of an utterance's results depends on the grid or on its neighbours.
#include "common.h"
#include "gemm_f32.h"
#include "gmm_tile.h"
#include "fixed_sum.h"
#include "utt_chain.h"
#include "vit_wave.h"
#include "../../include/abnet3_hip_next.h"

#include <math.h>

namespace abn {

static_assert(GM_B == UC_B, "utt_chain.h's geometry is these kernels'");
constexpr ChainLimits HM_LIMITS = {GM_MAX_D, "abn_gmm_max_d", GM_MAX_K, "abn_hmm_max_k", "abn_hmm_max_len"};
constexpr int64_t HM_FB_FRAME_BYTES = sizeof(float);      // forward-backward keeps c_t per frame

struct HmmP {
    GmmP g;                                 // x, shift, A, B, c = c0, T, K, D, tiles_k: a kernel argument, as in gmm.hip (the
                                            // loaders pick a table by the column's kind: from the kernarg segment, not a stack copy)
    const float* w;
    const int64_t* off; const int* len;
    int n_utt, mode;
    float rho;
    float* post; double* loglik; double* stays; int* n_good;
    double* stay_k;                         // [n_utt][K], the SK instantiations only
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, cap;                            // slab row stride (floats), frames the region holds
};

// The block of frames m0 .. m0 + nf - 1: BAD flags, the bt slab and m_t.  Ends behind a barrier.
__device__ __forceinline__ void hmm_block_scores(const HmmP& p, int m0, int nf, float* smem, float* slab,
                                                 const float* w_s, int* bad_s, float* mt_s)
{
    float* const As = smem;
    float* const Bs = smem + 2 * GmTile::floats;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int ks = p.ks;
    const GmmP& gp = p.g;
    if (t < GM_B) {
        bool bad = false;
        if (t < nf)
            for (int d = 0; d < gp.D; ++d) {
                const float xc = gp.x[(int64_t)(m0 + t) * gp.D + d] - gp.shift[d];
                bad |= !__builtin_isfinite(xc * xc);
            }
        bad_s[t] = bad;
    }
    for (int ct = 0; ct < gp.tiles_k; ++ct) {
        const int n0 = ct * GM_B;
        f32x16 acc[2][2];
        gmm_score_tile(gp, m0, n0, As, Bs, acc);
        const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    slab[(int64_t)(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * ks + n0 + wn0 + 32 * j + col_l] = acc[i][j][r];
    }
    __syncthreads();                                                  // the slab is this workgroup's own
    // wave w takes frames w, w + 4, ...: lanes over k
    for (int f = wave; f < nf; f += 4) {
        float* const row = slab + (int64_t)f * ks;
        float m = -INFINITY;
        for (int k = lane; k < gp.K; k += 64)
            if (w_s[k] > 0.0f) m = fmaxf(m, row[k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        for (int k = lane; k < gp.K; k += 64) row[k] = w_s[k] > 0.0f ? expf(row[k] - m) : 0.0f;
        if (lane == 0) mt_s[f] = m;
    }
    __syncthreads();
}

// SK: the per-component stays as well (abn_hmm_forward_backward_stats).  The chain, `post`, loglik, stays and n_good are
// the same instructions in the same order either way.  A thread adds its own components' terms ah e in fp32 over a block
// of 128 frames and then into stay_k[u][k] in float64: the row is the store of the float64 sums, every element is read and
// written by the one thread that owns it, and the factor rho is applied at the utterance's end.
template <int NQ, bool SK>
__global__ __launch_bounds__(256) void hmm_fb_kernel(HmmP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float w_s[GM_MAX_K];
    __shared__ int bad_s[GM_B];
    __shared__ float mt_s[GM_B], c_s[GM_B];
    __shared__ float red_s[2][4];
    __shared__ double red_d[256];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = reinterpret_cast<float*>(base);
    float* const cw = reinterpret_cast<float*>(base + (int64_t)sizeof(float) * GM_B * p.ks);
    const int ks = p.ks;
    const float rho = p.rho, omr = 1.0f - p.rho;
    const int K = p.g.K;

    for (int k = t; k < GM_MAX_K; k += 256) w_s[k] = k < K ? p.w[k] : 0.0f;      // (read per frame: the registers stay with the chain)
    __syncthreads();

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (o < 0 || L < 0 || o + L > p.g.T || L > p.cap) {          // (uniform) nothing of this utterance is touched
            if (t == 0) {
                p.loglik[u] = NAN;
                p.n_good[u] = -1;
                if (p.stays) p.stays[u] = NAN;
            }
            if constexpr (SK)
                for (int k = t; k < K; k += 256) p.stay_k[(int64_t)u * K + k] = NAN;
            continue;
        }
        double* const skrow = SK ? p.stay_k + (int64_t)u * K : nullptr;
        if constexpr (SK)
            for (int k = t; k < K; k += 256) skrow[k] = 0.0;          // (mode 1, fewer than two good frames: it stays 0)
        float* const post = p.post + o * K;
        float a[NQ], e[NQ];                                           // forward: ahat; backward: bhat and the later frame's e
#pragma unroll
        for (int q = 0; q < NQ; ++q) { a[q] = 0.0f; e[q] = 0.0f; }
        bool started = false;
        int ngood = 0, remaining = 0, par = 0;
        double ll = 0.0, st = 0.0;

        // Steps 0 .. nblk - 1: the forward sweep over the blocks; steps nblk .. 2 nblk - 1 (mode 0): the backward sweep,
        // last block first.  (One loop, so that the score phase is in the kernel once.)
        const int nblk = (L + GM_B - 1) / GM_B;
        const int nstep = p.mode == 0 ? 2 * nblk : nblk;
        for (int step = 0; step < nstep; ++step) {
            const bool fwd = step < nblk;
            if (step == nblk) {                                       // (uniform) the turn: bhat = 1 at the last good frame
                if (ngood < 2) break;                                 // gamma = ahat, no transition
                remaining = ngood;
#pragma unroll
                for (int q = 0; q < NQ; ++q) a[q] = 1.0f;
            }
            const int f0 = (fwd ? step : 2 * nblk - 1 - step) * GM_B;
            const int nf = min(GM_B, L - f0);
            if (!fwd && t < nf) c_s[t] = cw[f0 + t];                  // (thread 0's stores of the forward sweep, barriers behind)
            hmm_block_scores(p, (int)o + f0, nf, smem, slab, w_s, bad_s, mt_s);

            if (fwd) {
                float bn[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) bn[q] = 256 * q + t < K ? slab[256 * q + t] : 0.0f;
                for (int f = 0; f < nf; ++f) {
                    float b[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) b[q] = bn[q];
                    if (f + 1 < nf) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q) bn[q] = 256 * q + t < K ? slab[(int64_t)(f + 1) * ks + 256 * q + t] : 0.0f;
                    }
                    float* const prow = post + (int64_t)(f0 + f) * K;
                    if (bad_s[f]) {                                   // (uniform) the chain passes over it
#pragma unroll
                        for (int q = 0; q < NQ; ++q)
                            if (256 * q + t < K) prow[256 * q + t] = 0.0f;
                        continue;
                    }
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const float wk = w_s[256 * q + t];
                        b[q] *= started ? rho * a[q] + omr * wk : wk;
                        s += b[q];
                    }
                    s = fixed_wave_sum(s);
                    if (lane == 0) red_s[par][wave] = s;
                    __syncthreads();
                    const float c = ((red_s[par][0] + red_s[par][1]) + red_s[par][2]) + red_s[par][3];
                    par ^= 1;                                         // (the other set is not rewritten before the next barrier)
                    const float inv = 1.0f / c;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        a[q] = b[q] * inv;
                        if (256 * q + t < K) prow[256 * q + t] = a[q];
                    }
                    if (t == 0) { c_s[f] = c; cw[f0 + f] = c; }
                    started = true;
                    ++ngood;
                }
                __syncthreads();                                      // c_s is complete; the slab's readers are done
                double v = 0.0;
                if (t < nf && !bad_s[t]) v = log((double)c_s[t]) + (double)mt_s[t];
                ll += fixed_block_sum(v, red_d);
            } else {
                float bn[NQ], an[NQ];
                float sk[SK ? NQ : 1];
                if constexpr (SK) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) sk[q] = 0.0f;
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const bool in = 256 * q + t < K;
                    bn[q] = in ? slab[(int64_t)(nf - 1) * ks + 256 * q + t] : 0.0f;
                    an[q] = in ? post[(int64_t)(f0 + nf - 1) * K + 256 * q + t] : 0.0f;
                }
                for (int f = nf - 1; f >= 0; --f) {
                    float b[NQ], ah[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) { b[q] = bn[q]; ah[q] = an[q]; }
                    if (f > 0) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q) {
                            const bool in = 256 * q + t < K;
                            bn[q] = in ? slab[(int64_t)(f - 1) * ks + 256 * q + t] : 0.0f;
                            an[q] = in ? post[(int64_t)(f0 + f - 1) * K + 256 * q + t] : 0.0f;
                        }
                    }
                    if (bad_s[f]) continue;                           // (uniform)
                    float* const prow = post + (int64_t)(f0 + f) * K;
                    float sp = 0.0f;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        sp += ah[q] * e[q];                           // (e = 0 at the last good frame)
                        if (256 * q + t < K) prow[256 * q + t] = ah[q] * a[q];
                    }
                    st += (double)sp;
                    if constexpr (SK) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q) sk[q] += ah[q] * e[q];
                    }
                    if (--remaining == 0) break;                      // (uniform) the first good frame has no predecessor
                    const float inv = 1.0f / c_s[f];
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        e[q] = b[q] * a[q] * inv;
                        s += w_s[256 * q + t] * e[q];
                    }
                    s = fixed_wave_sum(s);
                    if (lane == 0) red_s[par][wave] = s;
                    __syncthreads();
                    const float tot = omr * (((red_s[par][0] + red_s[par][1]) + red_s[par][2]) + red_s[par][3]);
                    par ^= 1;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) a[q] = rho * e[q] + tot;
                }
                if constexpr (SK) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        if (256 * q + t < K) skrow[256 * q + t] += (double)sk[q];
                }
                __syncthreads();                                      // before the next block's scores replace these
                if (remaining == 0) break;                            // (uniform)
            }
        }
        if (p.stays) {                                                // (uniform)
            const double tot = fixed_block_sum(st, red_d);
            if (t == 0) p.stays[u] = (double)rho * tot;
        }
        if constexpr (SK)
            for (int k = t; k < K; k += 256) skrow[k] *= (double)rho;
        if (t == 0) {
            p.loglik[u] = ll;
            p.n_good[u] = ngood;
        }
        __syncthreads();
    }
}

// ---- abn_hmm_accumulate: sufficient statistics from a responsibility table ---------------------------------------------
// gmm_accum_kernel's second GEMM with the A operand LOADED: a workgroup owns a tile of 128 components and a range of
// frame blocks, [S1 | S2 | N][k][.] += sum_t post[t][k] X~[t][.] on the fp32 matrix cores, accumulators in registers for the
// whole range, one slab per workgroup.  The 128 x 128 tile of `post` (64 elements per thread: column t % 128 of rows
// t / 128 + 2 i, so a wave reads 64 consecutive components of a frame) is the launch's whole memory traffic, T K 4 bytes
// once: it is fetched one block ahead into registers, a quarter behind each of the four 32-frame steps of the block
// before, and committed k-major ([frame][132], zero past T and past K) once that block's last step has been read.  The
// X~ tiles stream in two LDS stages across the blocks.  LDS: 66 KiB + 2 x 32 x (BN + 4) floats, one workgroup per CU.
// gmm_xk_issue for a step whose 32 frames lie inside the table (uniform; every step but the table's last few): the same
// elements as ONE per-thread 32-bit offset on a uniform pointer per frame -- the clamped 64-bit form costs a dozen VALU
// instructions per element, and with one wave per SIMD they are not hidden behind anybody's MFMAs.
template <int BN>
__device__ __forceinline__ void hmm_xk_issue(float* r, const GmmP& p, int f0)
{
    if (f0 + BK > p.T) {
        gmm_xk_issue<BN>(r, p, f0);
        return;
    }
    constexpr int PT = 32 * BN / 256, FS = 256 / BN > 0 ? 256 / BN : 1;
    const int t = threadIdx.x, ka = t % BN, col = aug_col(ka, p.D);
    const bool kv = ka < 2 * p.D;
    const float* const base = p.x + (int64_t)f0 * p.D;
    const uint32_t toff = kv ? (uint32_t)((BN >= 256 ? 0 : t / BN) * p.D + col) : 0u;      // (a column of the fill: element 0)
#pragma unroll
    for (int i = 0; i < PT; ++i) r[i] = (base + (BN >= 256 ? i : FS * i) * p.D)[toff];
}

template <int BN> constexpr size_t hmm_accum_lds() { return sizeof(float) * (GM_B * GM_GST + 2 * TileShape<BN, false>::floats); }

template <int BN>
__global__ __launch_bounds__(256) void hmm_accum_kernel(GmmP p, const float* __restrict__ gamma)
{
    constexpr int TN = BN / 64, XPT = 32 * BN / 256, NS = GM_B / BK, GPT = GM_B * GM_B / 256, GPS = GPT / NS;
    using XT = TileShape<BN, false>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const G = smem;                                  // [128 frames][132]
    float* const Xk = smem + GM_B * GM_GST;                 // two stages of [32][BN + 4]

    const int total = p.tiles_k * p.n_ranges;               // (gmm_accum_kernel's order: a tile's ranges on one XCD)
    const int w = xcd_tile_index((int)blockIdx.x, total);
    const int ct = w / p.n_ranges, rg = w % p.n_ranges;
    const int n0 = ct * GM_B;
    const int b0 = rg * p.blocks_per_range, b1 = min(p.fblocks, b0 + p.blocks_per_range);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wc0 = (wave >> 1) * 64, wx0 = (wave & 1) * (BN / 2);   // statistics tile: components x columns
    const int col_l = lane & 31, rsub = 4 * (lane >> 5);
    const int gcl = t & (GM_B - 1), grl = t >> 7;
    const bool gcol = n0 + gcl < p.K;
    const int gcc = min(n0 + gcl, p.K - 1);                 // (past K: a valid address, the value is dropped at the commit)
    const uint32_t voff = (uint32_t)(grl * p.K + gcc);      // row t / 128 of a block; + 2 K per element

    f32x16 st[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[i][j][r] = 0.0f;

    // Elements i0 .. i0 + GPS - 1 of this thread's share of the block at frame mb.  A block inside the table (uniform; all
    // but the table's last): one per-thread 32-bit offset on a uniform pointer per row.  The last block: clamped addresses; validity is applied
    // at the commit either way.
    float rp[GPT], rx[XPT];
    const auto g_fetch = [&](int mb, int i0) {
        if (mb + GM_B <= p.T) {
            const float* const base = gamma + (int64_t)mb * p.K;
#pragma unroll
            for (int i = 0; i < GPS; ++i) rp[i0 + i] = (base + 2 * (i0 + i) * p.K)[voff];
        } else {
#pragma unroll
            for (int i = 0; i < GPS; ++i) {
                const int64_t fr = (int64_t)mb + grl + 2 * (i0 + i);
                rp[i0 + i] = gamma[fr < p.T ? fr * p.K + gcc : 0];
            }
        }
    };
    const auto frags = [&](const float* gs, const float* xs, int g, f32x4 (&fa)[2], f32x4 (&fx)[TN]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = frag_read<GM_B, false>(gs, wc0 + 32 * i, g, lane);
#pragma unroll
        for (int j = 0; j < TN; ++j) fx[j] = frag_read<BN, false>(xs, wx0 + 32 * j, g, lane);
    };
    hmm_xk_issue<BN>(rx, p, b0 * GM_B);
#pragma unroll
    for (int q = 0; q < NS; ++q) g_fetch(b0 * GM_B, q * GPS);
    gmm_xk_commit<BN>(rx, Xk, p, b0 * GM_B);

    for (int fb = b0; fb < b1; ++fb) {
        const int m0 = fb * GM_B;
        const bool nextb = fb + 1 < b1;
#pragma unroll
        for (int i = 0; i < GPT; ++i) {                     // (every wave is behind the barrier of the last block's last step)
            const int rl = grl + 2 * i;
            G[rl * GM_GST + gcl] = (gcol && m0 + rl < p.T) ? rp[i] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const float* const gs = G + q * BK * GM_GST;
            const float* const xs = Xk + (q & 1) * XT::floats;
            const bool more = q + 1 < NS || nextb;
            const int fnext = m0 + (q + 1) * BK;            // (q = NS - 1: the next block's first step)
            if (more) hmm_xk_issue<BN>(rx, p, fnext);
            if (nextb) g_fetch(m0 + GM_B, q * GPS);          // (uniform)
            // the fragments of k-group g + 1 are read before the MFMAs of group g are issued: with one wave per SIMD
            // nothing else covers the LDS latency
            f32x4 fa[2][2], fx[2][TN];
            frags(gs, xs, 0, fa[0], fx[0]);
#pragma unroll
            for (int g = 0; g < BK / 8; ++g) {
                if (g + 1 < BK / 8) frags(gs, xs, g + 1, fa[(g + 1) & 1], fx[(g + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            st[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][i][e], fx[g & 1][j][e], st[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (more) gmm_xk_commit<BN>(rx, Xk + ((q + 1) & 1) * XT::floats, p, fnext);
            __syncthreads();
        }
    }

    const int nc = 2 * p.D + 1;
    float* const slab = p.slabs + ((int64_t)ct * p.n_ranges + rg) * GM_B * nc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kl = wc0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub, col = wx0 + 32 * j + col_l;
                if (col < nc) slab[kl * nc + col] = st[i][j][r];
            }
}

// One workgroup per component: its slabs in range order, in float64 (gmm_reduce_kernel's component blocks).
__global__ __launch_bounds__(256) void hmm_sums_kernel(const float* __restrict__ slabs, int nc, int n_ranges,
                                                        double* __restrict__ sums)
{
    gmm_sum_slabs(slabs, (int)blockIdx.x, nc, n_ranges, sums);
}

// ---- max-product path (abn_hmm_viterbi) ----------------------------------------------------------------------------------
// The max-product twin of hmm_fb_kernel and the HMM twin of km_viterbi_kernel (kmeans.hip), whose shape it takes over:
// persistent workgroups, utterance u = blockIdx.x, + gridDim.x, ...  Per block of 128 frames the score tiles logN (the
// score phase of hmm_block_scores without the max / exp rewrite) go into the workgroup's own slab [128][ks] -- in LDS
// behind the operand tiles where K <= 128, otherwise in the workspace --, then one sequential step per frame: component
// k = 256 q + thread, W and the three log tables in registers, every operation one rounded add or a compare,
//   a = W + ls,  st = a > lr,  u = s + (st ? a : lr)   (first good frame: u = s + lw),   M = max u,  W = u - M,
// the max and its lowest index as ONE 64-bit max-reduction (vit_wave.h) and one LDS exchange, one ballot word of stay
// bits per 64 components, and the previous good frame's j* as an int32 (-1: the first good frame, -2: a BAD frame).
// Wave 0 then walks the stay bits backwards 64 frames at a time.  The slab, the stay bits and prevj are written and read
// by this workgroup alone with a workgroup barrier between, in 256-byte aligned regions: the comment above KM_VIT_LDS_KS
// (kmeans.hip) says why that is enough.
constexpr int HM_VIT_LDS_KS = GM_B + 8;    // K <= 128: slab rows 136 floats apart (the two half-waves of a deposit on different banks)
constexpr size_t HM_VIT_LDS_BYTES = GM_TILE_BYTES + sizeof(float) * GM_B * HM_VIT_LDS_KS;       // 140 KiB of the CU's 160
static_assert(HM_VIT_LDS_BYTES + 1024 <= 160 * 1024, "the LDS slab fits beside the operand tiles and the static arrays");

struct HmmVitP {
    GmmP g;                                 // x, shift, A, B, c = c0, T, K, D, tiles_k (a kernel argument, as in HmmP)
    const float* lw; const float* ls; const float* lr;
    const int64_t* off; const int* len;
    int n_utt;
    int* ids; double* log_prob; int* n_switch; int* n_good;
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, kw, cap;                        // slab row stride (floats), stay words per frame, frames the region holds
};

// The block of frames m0 .. m0 + nf - 1: BAD flags and the score tiles logN into the slab.  Ends behind a barrier.
// (hmm_block_scores' first half, restated: with one shared function hmm_fb_kernel measured 5 to 7 % slower, DESIGN.md
// section 3.4c2.)
__device__ __forceinline__ void hmm_vit_scores(const GmmP& gp, int m0, int nf, float* smem, float* slab, int ks, int* bad_s)
{
    float* const As = smem;
    float* const Bs = smem + 2 * GmTile::floats;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    if (t < GM_B) {
        bool bad = false;
        if (t < nf)
            for (int d = 0; d < gp.D; ++d) {
                const float xc = gp.x[(int64_t)(m0 + t) * gp.D + d] - gp.shift[d];
                bad |= !__builtin_isfinite(xc * xc);
            }
        bad_s[t] = bad;
    }
    for (int ct = 0; ct < gp.tiles_k; ++ct) {
        const int n0 = ct * GM_B;
        f32x16 acc[2][2];
        gmm_score_tile(gp, m0, n0, As, Bs, acc);
        const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    slab[(int64_t)(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * ks + n0 + wn0 + 32 * j + col_l] = acc[i][j][r];
    }
    __syncthreads();                                                  // the slab and bad_s are this workgroup's own
}

template <int NQ, bool LDSS>
__global__ __launch_bounds__(256) void hmm_viterbi_kernel(HmmVitP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int bad_s[GM_B];
    __shared__ unsigned long long red_k[2][4];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = LDSS ? smem + 4 * GmTile::floats : reinterpret_cast<float*>(base);
    const int ks = LDSS ? HM_VIT_LDS_KS : p.ks;
    unsigned long long* const stay = reinterpret_cast<unsigned long long*>(base + (int64_t)sizeof(float) * GM_B * p.ks);
    int* const prevj = reinterpret_cast<int*>(stay + (int64_t)p.cap * p.kw);
    const int K = p.g.K;

    float lw[NQ], ls[NQ], lr[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int k = 256 * q + t;
        lw[q] = k < K ? p.lw[k] : 0.0f;
        ls[q] = k < K ? p.ls[k] : 0.0f;
        lr[q] = k < K ? p.lr[k] : 0.0f;
    }

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (o < 0 || L < 0 || o + L > p.g.T || L > p.cap) {          // (uniform) nothing of this utterance is touched
            if (t == 0) {
                if (p.log_prob) p.log_prob[u] = NAN;
                if (p.n_switch) p.n_switch[u] = -1;
                if (p.n_good) p.n_good[u] = -1;
            }
            continue;
        }
        float W[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) W[q] = 0.0f;
        bool started = false;
        int jprev = -1, par = 0, ngood = 0;
        double lp = 0.0;

        for (int f0 = 0; f0 < L; f0 += GM_B) {
            const int nf = min(GM_B, L - f0);
            hmm_vit_scores(p.g, (int)o + f0, nf, smem, slab, ks, bad_s);

            float sn[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + t < K ? slab[256 * q + t] : 0.0f;
            for (int f = 0; f < nf; ++f) {
                const int g = f0 + f;
                float s[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q] = sn[q];
                if (f + 1 < nf) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + t < K ? slab[(int64_t)(f + 1) * ks + 256 * q + t] : 0.0f;
                }
                if (bad_s[f]) {                                       // (uniform) the chain passes over it
                    if (t == 0) prevj[g] = -2;
                    continue;
                }
                unsigned long long key = 0;                           // (below the key of -inf)
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int k = 256 * q + t;
                    const float a = W[q] + ls[q];
                    const bool st = started && a > lr[q];             // strict: a tie goes to the switch
                    const unsigned long long word = __ballot(st);
                    if (lane == 0) stay[(int64_t)g * p.kw + 4 * q + wave] = word;
                    float uq = s[q] + (started ? (st ? a : lr[q]) : lw[q]);
                    if (k >= K) uq = -INFINITY;
                    W[q] = uq;
                    const unsigned long long kq = vit_key(uq, k);
                    key = kq > key ? kq : key;
                }
                key = vit_wave_max(key);
                if (lane == 0) red_k[par][wave] = key;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long ok = red_k[par][w];
                    key = ok > key ? ok : key;
                }
                par ^= 1;                                             // (the other set is not rewritten before the next barrier)
                const float bv = vit_key_score(key);
                int bi = (int)~(unsigned)key;
                if ((unsigned)bi >= (unsigned)K) bi = 0;              // no score compared greater than -inf: still an id
#pragma unroll
                for (int q = 0; q < NQ; ++q) W[q] -= bv;
                lp += (double)bv;
                if (t == 0) prevj[g] = jprev;
                jprev = bi;
                started = true;
                ++ngood;
            }
            __syncthreads();                                          // before the next block's scores replace these
        }

        if (wave == 0) {                                              // traceback: jprev is the last good frame's j*
            const int nsw = vit_traceback(stay, prevj, p.kw, p.ids, o, L, jprev, lane);
            if (lane == 0) {
                if (p.log_prob) p.log_prob[u] = lp;
                if (p.n_switch) p.n_switch[u] = nsw;
                if (p.n_good) p.n_good[u] = ngood;
            }
        }
        __syncthreads();                                              // the traceback's reads before the next utterance's writes
    }
}

struct HmmVitKernels {
    template <int NQ, bool LDSS> static constexpr auto kernel() { return hmm_viterbi_kernel<NQ, LDSS>; }
};

// ---- max-product path with a minimum duration (abnx_hmm_viterbi_dur) -----------------------------------------------------
// hmm_viterbi_kernel's twin for the minimum-duration topology (vit_wave.h: every component a left-to-right chain of S
// states with tied emissions): the same persistent workgroups, score slab, stay words and prevj, and so the same
// workspace.  Thread t keeps the chains of its components in V[NQ][SC] registers, SC the capacity the kernel is
// instantiated with (the smallest of 1, 2, 4, 8 that holds S).  A frame needs two reductions before its one barrier: the
// keyed max over the exit states (E and the exit j*, which prevj records) and the max over all states (N_t).  After the
// last frame one more keyed max finds the final state, and wave 0 walks back with vit_traceback_dur.
struct HmmVitDurP { HmmVitP v; int S; };

template <int NQ, bool LDSS, int SC>
__global__ __launch_bounds__(256) void hmm_viterbi_dur_kernel(HmmVitDurP pd)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int bad_s[GM_B];
    __shared__ unsigned long long red_k[2][4];
    __shared__ float red_n[2][4];

    const HmmVitP& p = pd.v;
    const int S = pd.S, e0 = SC - S;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = LDSS ? smem + 4 * GmTile::floats : reinterpret_cast<float*>(base);
    const int ks = LDSS ? HM_VIT_LDS_KS : p.ks;
    unsigned long long* const stay = reinterpret_cast<unsigned long long*>(base + (int64_t)sizeof(float) * GM_B * p.ks);
    int* const prevj = reinterpret_cast<int*>(stay + (int64_t)p.cap * p.kw);
    const int K = p.g.K;
    constexpr int PARK = vit_dur_parked<NQ, SC>(LDSS);
    float* const park = smem + 4 * GmTile::floats;                    // behind the operand tiles (where the LDS slab would be)

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (o < 0 || L < 0 || o + L > p.g.T || L > p.cap) {          // (uniform) nothing of this utterance is touched
            if (t == 0) {
                if (p.log_prob) p.log_prob[u] = NAN;
                if (p.n_switch) p.n_switch[u] = -1;
                if (p.n_good) p.n_good[u] = -1;
            }
            continue;
        }
        float V[NQ][SC];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < SC; ++j) V[q][j] = -INFINITY;
        bool started = false;
        float E = 0.0f;
        int jprev = -1, par = 0, ngood = 0;
        double lp = 0.0;

        for (int f0 = 0; f0 < L; f0 += GM_B) {
            const int nf = min(GM_B, L - f0);
            vit_dur_park<PARK>(V, park, t);
            hmm_vit_scores(p.g, (int)o + f0, nf, smem, slab, ks, bad_s);
            vit_dur_unpark<PARK>(V, park, t);

            // The tables are read again per block, not kept across the score tile, and neither are the 4 NQ addresses of these
            // loads: tb is t behind an empty asm, so the compiler cannot hoist them out of the loops as invariants (it did,
            // and spilled them to scratch).
            int tb = t;
            asm volatile("" : "+v"(tb));
            float lw[NQ], ls[NQ], lr[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int k = 256 * q + tb;
                lw[q] = k < K ? p.lw[k] : 0.0f;
                ls[q] = k < K ? p.ls[k] : 0.0f;
                lr[q] = k < K ? p.lr[k] : 0.0f;
            }
            float sn[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + tb < K ? slab[256 * q + tb] : -INFINITY;
            for (int f = 0; f < nf; ++f) {
                const int g = f0 + f;
                float s[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q] = sn[q];
                if (f + 1 < nf) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + t < K ? slab[(int64_t)(f + 1) * ks + 256 * q + t] : -INFINITY;
                }
                if (bad_s[f]) {                                       // (uniform) the chain passes over it
                    if (t == 0) prevj[g] = -2;
                    continue;
                }
                unsigned long long key = 0;                           // (below the key of -inf)
                float nmax = -INFINITY;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {                        // (k >= K: s = -inf, so every state stays -inf)
                    const int k = 256 * q + t;
                    const float ent = started ? E + lr[q] : lw[q];
                    bool st;
                    const float m = vit_dur_step<SC>(V[q], s[q], ent, ls[q], e0, &st);
                    const unsigned long long word = __ballot(st);
                    if (lane == 0) stay[(int64_t)g * p.kw + 4 * q + wave] = word;
                    nmax = fmaxf(nmax, m);
                    const unsigned long long kq = vit_key(V[q][SC - 1], k);
                    key = kq > key ? kq : key;
                }
                key = vit_wave_max(key);
                if (SC > 1) nmax = vit_wave_fmax(nmax);
                if (lane == 0) {
                    red_k[par][wave] = key;
                    if (SC > 1) red_n[par][wave] = nmax;
                }
                __syncthreads();
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long ok = red_k[par][w];
                    key = ok > key ? ok : key;
                    if (SC > 1) nmax = fmaxf(nmax, red_n[par][w]);
                }
                par ^= 1;                                             // (the other set is not rewritten before the next barrier)
                const float xv = vit_key_score(key);
                const float nv = SC > 1 ? nmax : xv;                  // (one state per component: the exit max is the max)
                int bi = (int)~(unsigned)key;
                if ((unsigned)bi >= (unsigned)K) bi = 0;              // no score compared greater than -inf: still an id
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int j = 0; j < SC; ++j) V[q][j] -= nv;
                E = xv - nv;
                lp += (double)nv;
                if (t == 0) prevj[g] = jprev;
                jprev = bi;
                started = true;
                ++ngood;
            }
            __syncthreads();                                          // before the next block's scores replace these
        }

        int fcode = -1;                                               // the final state: the lowest k, then the largest slot, at 0
#pragma unroll
        for (int q = NQ - 1; q >= 0; --q) fcode = vit_dur_final_code<SC>(V[q], q, fcode);
        unsigned long long fkey = vit_wave_max(vit_dur_final_key<SC>(fcode, t));
        if (lane == 0) red_k[par][wave] = fkey;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned long long ok = red_k[par][w];
            fkey = ok > fkey ? ok : fkey;
        }

        if (wave == 0) {                                              // traceback from the final state
            int cur = -1, forced = 0;
            if (started && fkey) {
                cur = vit_dur_final_k(fkey);
                const int i = vit_dur_final_slot(fkey) - e0;
                forced = i == S - 1 ? 0 : i + 1;
            }
            const int nsw = vit_traceback_dur(stay, prevj, p.kw, p.ids, o, L, S, cur, forced, lane);
            if (lane == 0) {
                if (p.log_prob) p.log_prob[u] = lp;
                if (p.n_switch) p.n_switch[u] = nsw;
                if (p.n_good) p.n_good[u] = ngood;
            }
        }
        __syncthreads();                                              // the traceback's reads before the next utterance's writes
    }
}

template <int SC>
struct HmmVitDurKernels {
    template <int NQ, bool LDSS> static constexpr auto kernel() { return hmm_viterbi_dur_kernel<NQ, LDSS, SC>; }
};

}  // namespace abn

using namespace abn;

extern "C" int64_t abn_hmm_max_len(void) { return UC_MAX_LEN; }
extern "C" int64_t abn_hmm_max_k(void) { return GM_MAX_K; }

extern "C" int64_t abn_hmm_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D)
{
    return chain_ws_bytes("abn_hmm_ws_bytes", n_utt, max_len, K, D, HM_LIMITS, HM_FB_FRAME_BYTES, 0);
}

// Both forward-backward entries: `what` names the caller in the messages, stay_k != nullptr picks the SK kernels.
static int hmm_fb_launch(const char* what, const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len,
                         int64_t n_utt, const float* shift, const float* A, const float* B, const float* c0, const float* w,
                         int64_t K, float rho, int mode, float* post, double* loglik, double* stays, int32_t* n_good,
                         double* stay_k, void* ws, int64_t ws_bytes, void* stream)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - GM_B, "%s: T = %lld out of range", what, (long long)T);
    int rc = chain_check_sizes(what, n_utt, K, D, HM_LIMITS);
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && off && len && shift && A && B && c0 && w && post && loglik && n_good, "%s: null pointer", what);
    ABN_REQUIRE(rho >= 0.0f && rho < 1.0f, "%s: rho = %g, 0 <= rho < 1 is needed", what, (double)rho);
    ABN_REQUIRE(mode == 0 || mode == 1, "%s: mode = %d, 0 (smoothed) or 1 (filtered)", what, mode);
    const ChainWs hw = chain_ws(n_utt, 0, K, HM_FB_FRAME_BYTES, 0);
    ChainRegion a;
    rc = chain_region(what, "abn_hmm_ws_bytes", ws, ws_bytes, hw, &a);
    if (rc != ABN_OK) return rc;
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set))
        for_each_nq([](auto n) {
            chain_opt_in(reinterpret_cast<const void*>(hmm_fb_kernel<decltype(n)::value, false>), GM_TILE_BYTES);
            chain_opt_in(reinterpret_cast<const void*>(hmm_fb_kernel<decltype(n)::value, true>), GM_TILE_BYTES);
        });
    HmmP p;
    p.g = hmm_score_params(x, T, D, shift, A, B, c0, K);
    p.w = w; p.off = off; p.len = len; p.n_utt = (int)n_utt;
    p.mode = mode; p.rho = rho;
    p.post = post; p.loglik = loglik; p.stays = stays; p.n_good = n_good; p.stay_k = stay_k;
    p.ws = a.ws; p.per_wg = a.per_wg;
    p.ks = a.ks; p.cap = a.cap;
    const dim3 grid((unsigned)hw.grid);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nq = nq_for(K);
    for_each_nq([&](auto n) {
        if (decltype(n)::value != nq) return;
        if (stay_k) hipLaunchKernelGGL((hmm_fb_kernel<decltype(n)::value, true>), grid, dim3(256), GM_TILE_BYTES, st, p);
        else hipLaunchKernelGGL((hmm_fb_kernel<decltype(n)::value, false>), grid, dim3(256), GM_TILE_BYTES, st, p);
    });
    ABN_CHECK_LAUNCH(what);
    return ABN_OK;
}

extern "C" int abn_hmm_forward_backward(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len,
                                        int64_t n_utt, const float* shift, const float* A, const float* B, const float* c0,
                                        const float* w, int64_t K, float rho, int mode, float* post, double* loglik,
                                        double* stays, int32_t* n_good, void* ws, int64_t ws_bytes, void* stream)
{
    return hmm_fb_launch("abn_hmm_forward_backward", x, T, D, off, len, n_utt, shift, A, B, c0, w, K, rho, mode, post, loglik,
                         stays, n_good, nullptr, ws, ws_bytes, stream);
}

extern "C" int abn_hmm_forward_backward_stats(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len,
                                              int64_t n_utt, const float* shift, const float* A, const float* B,
                                              const float* c0, const float* w, int64_t K, float rho, int mode, float* post,
                                              double* loglik, double* stays, int32_t* n_good, double* stay_k, void* ws,
                                              int64_t ws_bytes, void* stream)
{
    ABN_REQUIRE(stay_k, "abn_hmm_forward_backward_stats: null pointer (stay_k)");
    return hmm_fb_launch("abn_hmm_forward_backward_stats", x, T, D, off, len, n_utt, shift, A, B, c0, w, K, rho, mode, post,
                         loglik, stays, n_good, stay_k, ws, ws_bytes, stream);
}

extern "C" int64_t abn_hmm_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D)
{
    return chain_ws_bytes("abn_hmm_viterbi_ws_bytes", n_utt, max_len, K, D, HM_LIMITS, vit_frame_bytes(K), 0);
}

// Both max-product entries: the checks in their order -- min_duration (null: the entry has none) behind the pointers --,
// the caller's workspace split into abn_hmm_viterbi_ws_bytes' regions, and the launch.  A min_duration of 1 launches the
// <1> instantiation of hmm_viterbi_dur_kernel, not hmm_viterbi_kernel: only abn_hmm_viterbi launches that one.
static int hmm_vit_run(const char* what, const int32_t* min_duration, const float* x, int64_t T, int64_t D, const int64_t* off,
                       const int32_t* len, int64_t n_utt, const float* shift, const float* A, const float* B, const float* c0,
                       const float* lw, const float* ls, const float* lr, int64_t K, int32_t* ids, double* log_prob,
                       int32_t* n_switch, int32_t* n_good, void* ws, int64_t ws_bytes, void* stream)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - GM_B, "%s: T = %lld out of range", what, (long long)T);
    int rc = chain_check_sizes(what, n_utt, K, D, HM_LIMITS);
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && off && len && shift && A && B && c0 && lw && ls && lr && ids, "%s: null pointer", what);
    const int S = min_duration ? *min_duration : 1;
    ABN_REQUIRE(S >= 1 && S <= VIT_DUR_MAX, "%s: min_duration = %d, 1 .. %d (abnx_viterbi_dur_max)", what, S, VIT_DUR_MAX);
    const ChainWs w = chain_ws(n_utt, 0, K, vit_frame_bytes(K), 0);
    ChainRegion a;
    rc = chain_region(what, "abn_hmm_viterbi_ws_bytes", ws, ws_bytes, w, &a);
    if (rc != ABN_OK) return rc;
    HmmVitDurP p;
    p.v.g = hmm_score_params(x, T, D, shift, A, B, c0, K);
    p.v.lw = lw; p.v.ls = ls; p.v.lr = lr; p.v.off = off; p.v.len = len; p.v.n_utt = (int)n_utt;
    p.v.ids = ids; p.v.log_prob = log_prob; p.v.n_switch = n_switch; p.v.n_good = n_good;
    p.v.ws = a.ws; p.v.per_wg = a.per_wg;
    p.v.ks = a.ks; p.v.kw = a.kw; p.v.cap = a.cap;
    p.S = S;
    if (!min_duration) return vit_launch<HmmVitKernels>(what, p.v, K, w, GM_TILE_BYTES, HM_VIT_LDS_BYTES, stream);
    return vit_dur_launch<HmmVitDurKernels>(what, p, S, K, w, GM_TILE_BYTES + VIT_DUR_PARK_BYTES, HM_VIT_LDS_BYTES, stream);
}

extern "C" int abn_hmm_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                               const float* shift, const float* A, const float* B, const float* c0, const float* lw,
                               const float* ls, const float* lr, int64_t K, int32_t* ids, double* log_prob, int32_t* n_switch,
                               int32_t* n_good, void* ws, int64_t ws_bytes, void* stream)
{
    return hmm_vit_run("abn_hmm_viterbi", nullptr, x, T, D, off, len, n_utt, shift, A, B, c0, lw, ls, lr, K, ids, log_prob,
                       n_switch, n_good, ws, ws_bytes, stream);
}

// abn_hmm_viterbi with a minimum duration (include/abnet3_hip_next.h); the workspace is abn_hmm_viterbi_ws_bytes'.
extern "C" int abnx_hmm_viterbi_dur(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                                    const float* shift, const float* A, const float* B, const float* c0, const float* lw,
                                    const float* ls, const float* lr, int64_t K, int32_t* ids, double* log_prob,
                                    int32_t* n_switch, int32_t* n_good, void* ws, int64_t ws_bytes, void* stream, int32_t min_duration)
{
    return hmm_vit_run("abnx_hmm_viterbi_dur", &min_duration, x, T, D, off, len, n_utt, shift, A, B, c0, lw, ls, lr, K, ids,
                       log_prob, n_switch, n_good, ws, ws_bytes, stream);
}

static int hmm_acc_check(int64_t T, int64_t K, int64_t D, int n_ranges, const char* what)
{
    ABN_REQUIRE(T >= 1 && K >= 1 && D >= 1, "%s: T = %lld, K = %lld, D = %lld out of range", what, (long long)T, (long long)K,
                (long long)D);
    ABN_REQUIRE(n_ranges >= 0 && n_ranges <= GM_MAX_RANGES, "%s: n_ranges = %d, supported 0 (by the grid) .. %d", what, n_ranges,
                GM_MAX_RANGES);
    if (D > GM_MAX_D || K > GM_MAX_K || T >= (1LL << 31) - GM_B) {
        set_error("%s: T = %lld, D = %lld, K = %lld, supported T < 2^31 - %d, D <= %d (abn_gmm_max_d), K <= %d (abn_hmm_max_k)",
                  what, (long long)T, (long long)D, (long long)K, GM_B, GM_MAX_D, GM_MAX_K);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

extern "C" int64_t abn_hmm_accumulate_ws_bytes(int64_t T, int64_t K, int64_t D, int n_ranges)
{
    if (hmm_acc_check(T, K, D, n_ranges, "abn_hmm_accumulate_ws_bytes") != ABN_OK) return -1;
    return gmm_slab_bytes(gmm_grid(T, K, n_ranges), D, n_ranges);
}

extern "C" int abn_hmm_accumulate(const float* x, int64_t T, int64_t D, const float* shift, const float* post, int64_t K,
                                  int n_ranges, double* sums, void* ws, int64_t ws_bytes, void* stream)
{
    const int rc = hmm_acc_check(T, K, D, n_ranges, "abn_hmm_accumulate");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && shift && post && sums, "abn_hmm_accumulate: null pointer");
    const GmmGrid g = gmm_grid(T, K, n_ranges);
    const int64_t need = gmm_slab_bytes(g, D, n_ranges);
    if (!ws || ws_bytes < need) {
        set_error("abn_hmm_accumulate: workspace of %lld bytes, %lld needed (abn_hmm_accumulate_ws_bytes)", (long long)ws_bytes,
                  (long long)need);
        return ABN_E_WORKSPACE;
    }
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_accum_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)hmm_accum_lds<64>());
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_accum_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)hmm_accum_lds<128>());
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_accum_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)hmm_accum_lds<256>());
    }
    GmmP p;
    p.x = x; p.shift = shift; p.A = nullptr; p.B = nullptr; p.c = nullptr;
    p.T = (int)T; p.K = (int)K; p.D = (int)D;
    p.lse = nullptr; p.post = nullptr; p.slabs = static_cast<float*>(ws);
    p.tiles_k = g.tiles_k; p.fblocks = g.fblocks; p.n_ranges = g.n_ranges; p.blocks_per_range = g.blocks_per_range;
    const dim3 grid((unsigned)(g.tiles_k * g.n_ranges));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nc = 2 * (int)D + 1;
    if (nc <= 64) hipLaunchKernelGGL(hmm_accum_kernel<64>, grid, dim3(256), hmm_accum_lds<64>(), st, p, post);
    else if (nc <= 128) hipLaunchKernelGGL(hmm_accum_kernel<128>, grid, dim3(256), hmm_accum_lds<128>(), st, p, post);
    else hipLaunchKernelGGL(hmm_accum_kernel<256>, grid, dim3(256), hmm_accum_lds<256>(), st, p, post);
    ABN_CHECK_LAUNCH("abn_hmm_accumulate");
    hipLaunchKernelGGL(hmm_sums_kernel, dim3((unsigned)K), dim3(256), 0, st, static_cast<const float*>(ws), nc, g.n_ranges, sums);
    ABN_CHECK_LAUNCH("abn_hmm_accumulate (sum)");
    return ABN_OK;
}
