// hmm.hip -- forward-backward of the sticky HMM over a mixture's components (abn_hmm_forward_backward).
// abnet3_amd/hmm.py states the definition; DESIGN.md section 3.4c2 the shape.
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

#include <math.h>

namespace abn {

constexpr int HM_GRID = 256;               // one workgroup per CU (the score tile keeps the register file to itself)
constexpr int HM_MAX_LEN = 1 << 20;

struct HmmP {
    GmmP g;                                 // x, shift, A, B, c = c0, T, K, D, tiles_k: a kernel argument, as in gmm.hip (the
                                            // loaders pick a table by the column's kind: from the kernarg segment, not a stack copy)
    const float* w;
    const int64_t* off; const int* len;
    int n_utt, mode;
    float rho;
    float* post; double* loglik; double* stays; int* n_good;
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, cap;                            // slab row stride (floats), frames the region holds
};

struct HmmWs { int64_t slab_bytes, per_wg; int grid, ks; };
static HmmWs hmm_ws(int64_t n_utt, int64_t max_len, int64_t K)
{
    HmmWs w;
    w.grid = (int)(n_utt < HM_GRID ? n_utt : HM_GRID);
    w.ks = (int)((K + GM_B - 1) / GM_B) * GM_B;
    w.slab_bytes = (int64_t)sizeof(float) * GM_B * w.ks;
    w.per_wg = align_up(w.slab_bytes + max_len * (int64_t)sizeof(float), 256);
    return w;
}

// One DPP exchange inside the rows of 16 lanes (every lane has a source under these controls) and the sum of the two:
// both partners add the same two numbers, so they hold the same bits.
template <int CTRL>
__device__ __forceinline__ float hmm_dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// The sum over the wave, in every lane, in one fixed order: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror leave the row's sum in its 16 lanes; the four rows' sums are read with v_readlane and added row 0 first.
// All 64 lanes must be active.
__device__ __forceinline__ float hmm_wave_sum(float v)
{
    v = hmm_dpp_add<0xB1>(v);
    v = hmm_dpp_add<0x4E>(v);
    v = hmm_dpp_add<0x141>(v);
    v = hmm_dpp_add<0x140>(v);
    float r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
#pragma unroll
    for (int i = 1; i < 4; ++i) r += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * i));
    return r;
}

// 256 doubles summed in a fixed tree; the result is returned to every thread.
__device__ __forceinline__ double hmm_block_sum(double v, double* sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

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

template <int NQ>
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
            continue;
        }
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
                    s = hmm_wave_sum(s);
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
                ll += hmm_block_sum(v, red_d);
            } else {
                float bn[NQ], an[NQ];
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
                    if (--remaining == 0) break;                      // (uniform) the first good frame has no predecessor
                    const float inv = 1.0f / c_s[f];
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        e[q] = b[q] * a[q] * inv;
                        s += w_s[256 * q + t] * e[q];
                    }
                    s = hmm_wave_sum(s);
                    if (lane == 0) red_s[par][wave] = s;
                    __syncthreads();
                    const float tot = omr * (((red_s[par][0] + red_s[par][1]) + red_s[par][2]) + red_s[par][3]);
                    par ^= 1;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) a[q] = rho * e[q] + tot;
                }
                __syncthreads();                                      // before the next block's scores replace these
                if (remaining == 0) break;                            // (uniform)
            }
        }
        if (p.stays) {                                                // (uniform)
            const double tot = hmm_block_sum(st, red_d);
            if (t == 0) p.stays[u] = (double)rho * tot;
        }
        if (t == 0) {
            p.loglik[u] = ll;
            p.n_good[u] = ngood;
        }
        __syncthreads();
    }
}

static int hmm_check_sizes(int64_t n_utt, int64_t K, int64_t D, const char* what)
{
    ABN_REQUIRE(n_utt >= 1 && n_utt < (1LL << 31), "%s: n_utt = %lld out of range", what, (long long)n_utt);
    ABN_REQUIRE(K >= 1 && D >= 1, "%s: K = %lld, D = %lld out of range", what, (long long)K, (long long)D);
    if (D > GM_MAX_D || K > GM_MAX_K) {
        set_error("%s: D = %lld, K = %lld, supported D <= %d (abn_gmm_max_d), K <= %d (abn_hmm_max_k)", what, (long long)D,
                  (long long)K, GM_MAX_D, GM_MAX_K);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abn_hmm_max_len(void) { return HM_MAX_LEN; }
extern "C" int64_t abn_hmm_max_k(void) { return GM_MAX_K; }

extern "C" int64_t abn_hmm_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D)
{
    if (hmm_check_sizes(n_utt, K, D, "abn_hmm_ws_bytes") != ABN_OK) return -1;
    if (max_len < 0 || max_len > HM_MAX_LEN) {
        set_error("abn_hmm_ws_bytes: max_len = %lld, supported 0 .. %d (abn_hmm_max_len)", (long long)max_len, HM_MAX_LEN);
        return -1;
    }
    const HmmWs w = hmm_ws(n_utt, max_len, K);
    return w.per_wg * w.grid;
}

extern "C" int abn_hmm_forward_backward(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len,
                                        int64_t n_utt, const float* shift, const float* A, const float* B, const float* c0,
                                        const float* w, int64_t K, float rho, int mode, float* post, double* loglik,
                                        double* stays, int32_t* n_good, void* ws, int64_t ws_bytes, void* stream)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - GM_B, "abn_hmm_forward_backward: T = %lld out of range", (long long)T);
    const int rc = hmm_check_sizes(n_utt, K, D, "abn_hmm_forward_backward");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && off && len && shift && A && B && c0 && w && post && loglik && n_good,
                "abn_hmm_forward_backward: null pointer");
    ABN_REQUIRE(rho >= 0.0f && rho < 1.0f, "abn_hmm_forward_backward: rho = %g, 0 <= rho < 1 is needed", (double)rho);
    ABN_REQUIRE(mode == 0 || mode == 1, "abn_hmm_forward_backward: mode = %d, 0 (smoothed) or 1 (filtered)", mode);
    const HmmWs hw = hmm_ws(n_utt, 0, K);
    const int64_t per_wg = ws_bytes > 0 ? (ws_bytes / hw.grid) & ~255LL : 0;
    int64_t cap = (per_wg - hw.slab_bytes) / (int64_t)sizeof(float);
    if (!ws || cap < 1) {
        set_error("abn_hmm_forward_backward: workspace of %lld bytes holds no frame (abn_hmm_ws_bytes)", (long long)ws_bytes);
        return ABN_E_WORKSPACE;
    }
    ABN_REQUIRE(aligned16(ws), "abn_hmm_forward_backward: the workspace must be 16-byte aligned");
    if (cap > HM_MAX_LEN) cap = HM_MAX_LEN;
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set)) {
        const auto opt_in = [](const void* k) { (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GM_TILE_BYTES); };
        opt_in(reinterpret_cast<const void*>(hmm_fb_kernel<1>));
        opt_in(reinterpret_cast<const void*>(hmm_fb_kernel<2>));
        opt_in(reinterpret_cast<const void*>(hmm_fb_kernel<4>));
        opt_in(reinterpret_cast<const void*>(hmm_fb_kernel<8>));
        opt_in(reinterpret_cast<const void*>(hmm_fb_kernel<16>));
    }
    HmmP p;
    p.g.x = x; p.g.shift = shift; p.g.A = A; p.g.B = B; p.g.c = c0;
    p.g.T = (int)T; p.g.K = (int)K; p.g.D = (int)D;
    p.g.lse = nullptr; p.g.post = nullptr; p.g.slabs = nullptr;
    p.g.tiles_k = (int)((K + GM_B - 1) / GM_B); p.g.fblocks = 0; p.g.n_ranges = 0; p.g.blocks_per_range = 0;
    p.w = w; p.off = off; p.len = len; p.n_utt = (int)n_utt;
    p.mode = mode; p.rho = rho;
    p.post = post; p.loglik = loglik; p.stays = stays; p.n_good = n_good;
    p.ws = static_cast<char*>(ws); p.per_wg = per_wg;
    p.ks = hw.ks; p.cap = (int)cap;
    const dim3 grid((unsigned)hw.grid);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int nq = 1;
    while (nq * 256 < K) nq <<= 1;
    switch (nq) {
    case 1: hipLaunchKernelGGL(hmm_fb_kernel<1>, grid, dim3(256), GM_TILE_BYTES, st, p); break;
    case 2: hipLaunchKernelGGL(hmm_fb_kernel<2>, grid, dim3(256), GM_TILE_BYTES, st, p); break;
    case 4: hipLaunchKernelGGL(hmm_fb_kernel<4>, grid, dim3(256), GM_TILE_BYTES, st, p); break;
    case 8: hipLaunchKernelGGL(hmm_fb_kernel<8>, grid, dim3(256), GM_TILE_BYTES, st, p); break;
    default: hipLaunchKernelGGL(hmm_fb_kernel<16>, grid, dim3(256), GM_TILE_BYTES, st, p); break;
    }
    ABN_CHECK_LAUNCH("abn_hmm_forward_backward");
    return ABN_OK;
}
