// hmm_hsmm.hip -- the hidden semi-Markov decoder over the full-transition model's units (abnu_hmm_hsmm_viterbi) and the run
// statistics that train its duration tables (abnu_hmm_run_stats); include/abnet3_hip_next.h, sixth section.
// abnet3_amd/hmm.py states the definition, tests/hmm_hsmm_np.py restates it; DESIGN.md section 3.4c10 the shape.
//
// hmm_dense_dur_kernel's launch shape (hmm_dense_vit.hip): one launch for the corpus, persistent workgroups with the static
// utterance assignment, the 128-frame slab of raw scores from the mixture's fp32 MFMA tile, lx in LDS as [KC][KC + 1] with
// -inf in the padding and on the diagonal, the K' x K' max-plus candidates in slices over 256 threads with the strict
// combine, one 64-bit key reduction per frame for N_t, the traceback in the same launch.  What is new:
//   * unit k has L duration states, L a run-time value 2 .. 32: the owner lane keeps the chain's normalised values V and the
//     unit's ld row in LC >= L registers each (LC = 8, 16 or 32), state i in slot LC - L + i - 1.  So the tail state L is
//     always slot LC - 1, the entry state 1 is slot e0 = LC - L (a uniform compare), the slots below e0 hold -inf for good,
//     and the frame's step is vit_wave.h's vit_dur_step with S = L: a shift, the entry, and the tail's stay-or-advance.
//   * what leaves unit j is not its last state but x[j] = max_i (V[j][i] + ld[j][i]) over the NORMALISED values, with xi[j]
//     the lowest i of the maximum.  It can be formed only behind the frame's key reduction, so a frame has a third barrier:
//     behind the partial pairs, behind the wave keys, behind x.  u_s holds x; nothing is subtracted by the readers.
//   * two bytes per (frame, unit): the backpointer in bits 0 .. 6 with the tail's stay bit in bit 7, and xi[unit] as it stood
//     when the frame was entered (1 .. L; 0 at the first good frame).  Two planes [128][KC] over the dead operand tiles; a
//     region of the workspace is  slab | [cap][KC] backpointers | [cap][KC] xi | [cap] BAD bytes.
//   * the utterance ends with one more key reduction over x: F = max_k x[k], the lowest k, and that owner's xi.
// Padding never wins (hmm_dense_vit.hip's argument: -inf + -inf loses every strict compare against slice 0's j = 0, and a
// thread that owns no unit puts no key into a reduction).  No floating-point atomic, fixed orders throughout, nothing of an
// utterance's results depends on the grid or on its neighbours.
//
// LDS at KC = 128: 72 KiB of operand tiles (the two byte planes, 32 KiB, lie over them) + 64.5 KiB of lx + about 4.6 KiB of
// static arrays, of the CU's 160 KiB -- hmm_dense_vit.hip's budget, hd_lds_bytes(KC) with its static_assert.
//
// Of hmm_dense.h's device layer the kernel takes the score block alone (hd_logn_block: the same function it had as its
// own), and HsmmP stays flat: its twelve instantiations compile to the instructions they had before that layer existed.
// Measured against that build at (D, K, L) = (40, 64, 8), 10.53 ms, band 0.3 %: every phase through shared functions
// 1.016 to 1.019 x; the plane copies in the kernel's own text 1.007; beside them the entry maximum 1.022, the key reduction
// 1.020, everything else 1.026 (all with HsmmP embedding HmmDenseVitP); the flat HsmmP with the shared phases 1.009: no
// mixture that was tried met the band (profiles/hmm_dense_shared_layer.md).  The host side below is hmm_dense.h's.
#include "common.h"
#include "gemm_f32.h"
#include "gmm_tile.h"
#include "utt_chain.h"
#include "vit_wave.h"
#include "hmm_dense.h"
#include "../../include/abnet3_hip_next.h"

#include <math.h>

namespace abn {

constexpr int HS_MAX_L = 32;
constexpr unsigned char HS_STAY = 0x80;
static_assert(HD_MAX_K <= HS_STAY, "a backpointer is seven bits beside the stay bit");
static_assert(HS_MAX_L < 256, "xi is one byte");
static_assert((size_t)2 * GM_B * HD_MAX_K <= GM_TILE_BYTES, "a block's two byte planes fit over the operand tiles");

struct HsmmP {
    GmmP g;                                 // x, shift, A, B, c = c0, T, K, D, tiles_k
    const float* li; const float* lx; const float* ld; const float* ls;
    const int64_t* off; const int* len;
    int n_utt, L;
    int* ids; double* log_prob; int* n_switch; int* n_good;
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, cap;                            // slab row stride (floats), frames the region holds
};

template <int KC, int LC>
__global__ __launch_bounds__(256) void hmm_hsmm_kernel(HsmmP p)
{
    constexpr int NS = 256 / KC, SW = KC / NS, TS = KC + 1;
    static_assert(NS * SW == KC && NS * KC == 256, "256 threads cover KC x KC in slices of SW");
    static_assert(LC >= 2 && LC <= HS_MAX_L, "the chain of a unit is held in LC registers");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int bad_s[GM_B];
    __shared__ int ids_s[GM_B];
    __shared__ unsigned long long red_k[4];
    __shared__ float part_v[256];                                     // [slice][own]
    __shared__ int part_j[256];
    __shared__ float u_s[KC];                                         // x of the previous good frame; -inf past K
    __shared__ int fin_s;                                             // the final unit's duration state

    float* const lx_s = smem + 4 * GmTile::floats;                    // [KC][TS], behind the operand tiles; the diagonal -inf
    unsigned char* const bp_s = reinterpret_cast<unsigned char*>(smem);      // [128][KC], over the operand tiles
    unsigned char* const xi_s = bp_s + GM_B * KC;                     // [128][KC] behind them
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int own = t % KC, sl = t / KC;
    const int K = p.g.K, ks = p.ks, L = p.L;
    const int e0 = LC - L;                                            // state i lives in slot e0 + i - 1
    const bool owner = t < K;                                         // unit t's chain is kept by this thread
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = reinterpret_cast<float*>(base);
    unsigned char* const bpw = reinterpret_cast<unsigned char*>(base + (int64_t)sizeof(float) * GM_B * ks);
    unsigned char* const xiw = bpw + (int64_t)p.cap * KC;
    unsigned char* const badw = xiw + (int64_t)p.cap * KC;

    for (int i = t; i < KC * TS; i += 256) {
        const int j = i / TS, k = i % TS;
        lx_s[i] = (j < K && k < K && j != k) ? p.lx[j * K + k] : -INFINITY;
    }
    if (t < KC) u_s[t] = -INFINITY;
    const float li = owner ? p.li[t] : 0.0f;
    const float ls = owner ? p.ls[t] : 0.0f;
    float ldr[LC];                                                    // the unit's ld row in the chain's slots (0 below e0, where V is -inf)
#pragma unroll
    for (int i = 0; i < LC; ++i) ldr[i] = (owner && i >= e0) ? p.ld[t * L + (i - e0)] : 0.0f;
    __syncthreads();

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int n = p.len[u];
        if (o < 0 || n < 0 || o + n > p.g.T || n > p.cap) {          // (uniform) nothing of this utterance is touched
            if (t == 0) {
                if (p.log_prob) p.log_prob[u] = NAN;
                if (p.n_switch) p.n_switch[u] = -1;
                if (p.n_good) p.n_good[u] = -1;
            }
            continue;
        }
        bool started = false;
        int ngood = 0;
        float V[LC];                                                  // the chain of unit t, normalised
#pragma unroll
        for (int i = 0; i < LC; ++i) V[i] = -INFINITY;
        float xv = -INFINITY;                                         // x[t] of the last good frame
        int xi = 0;                                                   // and its state, 1 .. L (0: no good frame yet)
        double lp = 0.0;
        const int nblk = (n + GM_B - 1) / GM_B;

        for (int b = 0; b < nblk; ++b) {
            const int f0 = b * GM_B;
            const int nf = min(GM_B, n - f0);
            hd_logn_block(p.g, (int)o + f0, nf, smem, slab, ks, bad_s);

            float sn = owner ? slab[t] : 0.0f;
            for (int f = 0; f < nf; ++f) {
                const float s = sn;
                if (f + 1 < nf) sn = owner ? slab[(int64_t)(f + 1) * ks + t] : 0.0f;
                if (bad_s[f]) continue;                               // (uniform) the chain passes over it
                float c = li;                                         // what enters state 1
                int bj = t;                                           // the first good frame: bp[k] = k
                if (started) {                                        // (uniform) c[own] = max_{j != own} x[j] + lx[j][own]
                    const float* const ltc = lx_s + (sl * SW) * TS + own;
                    const float* const uv = u_s + sl * SW;
                    float best = uv[0] + ltc[0];
                    int bc = 0;
#pragma unroll
                    for (int q = 1; q < SW; ++q) {
                        const float v = uv[q] + ltc[q * TS];
                        if (v > best) { best = v; bc = q; }           // strict: the lowest j on ties
                    }
                    part_v[t] = best;
                    part_j[t] = sl * SW + bc;
                    __syncthreads();
                    if (t < KC) {                                     // (sl == 0, own == t) slice 0 first, strictly
                        c = part_v[t];
                        bj = part_j[t];
#pragma unroll
                        for (int q = 1; q < NS; ++q) {
                            const float v = part_v[q * KC + t];
                            if (v > c) { c = v; bj = part_j[q * KC + t]; }
                        }
                    }
                }
                unsigned long long key = 0;                           // (below the key of -inf: the padding never wins)
                if (owner) {
                    bool st;
                    const float m = vit_dur_step<LC>(V, s, c, ls, e0, &st);
                    bp_s[f * KC + t] = (unsigned char)(bj | (st ? HS_STAY : 0));
                    xi_s[f * KC + t] = (unsigned char)xi;             // xi[t] as this frame's candidates read it
                    key = vit_key(m, t);
                }
                key = vit_wave_max(key);
                if (lane == 0) red_k[wave] = key;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long ok = red_k[w];
                    key = ok > key ? ok : key;
                }
                const float N = vit_key_score(key);
                lp += (double)N;
                if (owner) {                                          // V = U - N, then the exit maximum over it
                    int slot = 0;
#pragma unroll
                    for (int i = 0; i < LC; ++i) {
                        V[i] = V[i] - N;
                        const float v = V[i] + ldr[i];
                        if (i == 0) xv = v;
                        else if (v > xv) { xv = v; slot = i; }        // strict, ascending: the lowest state of the maximum
                    }
                    xi = max(slot - e0, 0) + 1;
                    u_s[t] = xv;
                }
                __syncthreads();                                      // x before the next frame's candidates; red_k, part_* free again
                started = true;
                ++ngood;
            }
            __syncthreads();                                          // the block's bytes are complete; the slab's readers are done
            if (b + 1 < nblk) {                                       // (uniform; nf == 128) the last block stays in LDS
                const unsigned* const src = reinterpret_cast<const unsigned*>(bp_s);
                unsigned* const dst = reinterpret_cast<unsigned*>(bpw + (int64_t)f0 * KC);
                unsigned* const dsx = reinterpret_cast<unsigned*>(xiw + (int64_t)f0 * KC);
                for (int i = t; i < GM_B * KC / 4; i += 256) {
                    dst[i] = src[i];
                    dsx[i] = src[GM_B * KC / 4 + i];
                }
                if (t < GM_B) badw[f0 + t] = (unsigned char)bad_s[t];
                __syncthreads();                                      // before the next block's operands replace them
            }
        }

        // The end of the utterance: F = max_k x[k], the lowest k, and that owner's xi.  Then the traceback, last block first;
        // cur, ci and nsw live in thread 0.
        int cur = -1, ci = 0, nsw = 0;
        if (ngood > 0) {                                              // (uniform)
            unsigned long long key = owner ? vit_key(xv, t) : 0;
            key = vit_wave_max(key);
            if (lane == 0) red_k[wave] = key;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned long long ok = red_k[w];
                key = ok > key ? ok : key;
            }
            lp += (double)vit_key_score(key);
            cur = (int)~(unsigned)key;
            if ((unsigned)cur >= (unsigned)K) cur = 0;                // no score compared greater than -inf: still an id
            if (t == cur) fin_s = xi;
            __syncthreads();
            ci = fin_s;
        }
        for (int b = nblk - 1; b >= 0; --b) {
            const int f0 = b * GM_B;
            const int nf = min(GM_B, n - f0);
            if (b + 1 < nblk) {                                       // (uniform; nf == 128)
                const unsigned* const src = reinterpret_cast<const unsigned*>(bpw + (int64_t)f0 * KC);
                const unsigned* const srx = reinterpret_cast<const unsigned*>(xiw + (int64_t)f0 * KC);
                unsigned* const dst = reinterpret_cast<unsigned*>(bp_s);
                for (int i = t; i < GM_B * KC / 4; i += 256) {
                    dst[i] = src[i];
                    dst[GM_B * KC / 4 + i] = srx[i];
                }
                if (t < GM_B) bad_s[t] = badw[f0 + t];
                __syncthreads();
            }
            if (t == 0) {
                for (int f = nf - 1; f >= 0; --f) {
                    if (bad_s[f] || cur < 0) {
                        ids_s[f] = -1;
                        continue;
                    }
                    ids_s[f] = cur;
                    const int byte = bp_s[f * KC + cur];
                    if (ci == L && (byte & HS_STAY)) continue;        // the tail repeats
                    if (ci > 1) { --ci; continue; }                   // inside the segment's head
                    const int pj = byte & (HS_STAY - 1);              // state 1: entered from pj in its state xi[pj]
                    nsw += pj != cur;                                 // (the first good frame holds bp[k] = k)
                    cur = pj;
                    ci = xi_s[f * KC + pj];
                }
            }
            __syncthreads();
            if (t < nf) p.ids[o + f0 + t] = ids_s[t];
        }
        if (t == 0) {
            if (p.log_prob) p.log_prob[u] = lp;
            if (p.n_switch) p.n_switch[u] = nsw;
            if (p.n_good) p.n_good[u] = ngood;
        }
        __syncthreads();                                              // the traceback's reads before the next utterance's writes
    }
}

// ---- the run statistics (abnu_hmm_run_stats) ---------------------------------------------------------------------------------
// hh_trans_kernel's shape (hmm_hard.hip): one wavefront per utterance, 64 ids at a time, the good lanes from a ballot.  The
// run that is open at the end of a chunk travels to the next one as (id, length) in two wave-uniform registers, so a run
// may cross any number of chunk edges and BAD frames.  A lane whose id differs from the previous good id closes that
// id's run: its length is the distance, in good frames, to the run's first lane (or to the chunk's start plus what was
// carried).  The counts go into an int32 [K][L + 1] table in LDS (column L: the tail frames) and are flushed once per
// workgroup with 64-bit integer atomics: integers, so any grid and any order give the same counts.
constexpr int HS_RUN_GRID = 256;
constexpr size_t hs_run_lds(int64_t K, int64_t L) { return sizeof(int) * (size_t)K * (size_t)(L + 1); }
static_assert(hs_run_lds(HD_MAX_K, HS_MAX_L) <= 64 * 1024, "the count table fits the LDS without an opt-in");

struct HsRunP {
    const int* ids; const int64_t* off; const int* len;
    int64_t T;
    int K, L, n_utt;
    unsigned long long* dur;      // [K][L]
    unsigned long long* tail;     // [K]
};

__device__ __forceinline__ void hs_run_add(int* tab, int L, int k, int n)
{
    atomicAdd(&tab[k * (L + 1) + (n < L ? n : L) - 1], 1);
    if (n > L) atomicAdd(&tab[k * (L + 1) + L], n - L);
}

__global__ __launch_bounds__(256) void hs_run_kernel(HsRunP p)
{
    extern __shared__ __attribute__((aligned(16))) int hs_tab[];      // [K][L + 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K, L = p.L, cells = K * (L + 1);
    for (int i = threadIdx.x; i < cells; i += 256) hs_tab[i] = 0;
    __syncthreads();

    const unsigned long long lt_mask = (1ull << lane) - 1ull;         // the lanes below this one
    for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < p.n_utt; u += (int64_t)gridDim.x * 4) {
        const int64_t o = p.off[u];
        const int n = p.len[u];
        if (o < 0 || n < 0 || o + n > p.T || n > UC_MAX_LEN) continue;      // refused: nothing added
        int cid = -1, clen = 0;                                       // (uniform) the open run
        for (int base = 0; base < n; base += 64) {
            const bool in = base + lane < n;
            const int id = in ? p.ids[o + base + lane] : -1;
            const bool good = in && id >= 0 && id < K;
            const unsigned long long mask = __ballot(good);
            if (!mask) continue;                                      // (uniform)
            const unsigned long long below = mask & lt_mask;
            const int rank = __popcll(below);                         // good frames of the chunk before this lane
            const int pl = below ? 63 - __builtin_clzll(below) : 0;
            const int pv = __shfl(id, pl);                            // (every lane takes the shuffle)
            const int prev = below ? pv : cid;                        // the previous good id, -1: none
            const bool start = good && prev != id;
            const unsigned long long smask = __ballot(start);
            if (start && prev >= 0) {                                 // prev's run ends in front of this lane
                const unsigned long long sb = smask & lt_mask;
                int len_run = rank + clen;                            // open since before the chunk
                if (sb) len_run = rank - __popcll(mask & ((1ull << (63 - __builtin_clzll(sb))) - 1ull));
                hs_run_add(hs_tab, L, prev, len_run);
            }
            const int cnt = __popcll(mask);
            if (smask) {                                              // (uniform) the chunk's last start opens the run carried on
                const int j = 63 - __builtin_clzll(smask);
                cid = __shfl(id, j);
                clen = cnt - __popcll(mask & ((1ull << j) - 1ull));
            } else clen += cnt;
        }
        if (lane == 0 && cid >= 0) hs_run_add(hs_tab, L, cid, clen);  // the utterance's last run
    }

    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += 256) {
        const int c = hs_tab[i];
        if (!c) continue;
        const int k = i / (L + 1), d = i % (L + 1);
        if (d < L) atomicAdd(&p.dur[k * L + d], (unsigned long long)c);      // integer: any order gives the same count
        else atomicAdd(&p.tail[k], (unsigned long long)c);
    }
}

}  // namespace abn

using namespace abn;

static int hs_check_L(const char* what, int32_t L)
{
    ABN_REQUIRE(L >= 2 && L <= HS_MAX_L, "%s: L = %d, 2 .. %d (abnu_hmm_hsmm_max_duration)", what, (int)L, HS_MAX_L);
    return ABN_OK;
}

extern "C" int32_t abnu_hmm_hsmm_max_duration(void) { return HS_MAX_L; }

extern "C" int64_t abnu_hmm_hsmm_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D, int32_t L)
{
    const char* what = "abnu_hmm_hsmm_viterbi_ws_bytes";
    if (hs_check_L(what, L) != ABN_OK) return -1;
    return chain_ws_bytes(what, n_utt, max_len, K, D, HD_LIMITS, hd_frame_bytes(K, 2, true), 0);
}

template <int LC>
static void hs_launch(const HsmmP& p, int kc, int grid, hipStream_t st)
{
    hd_for_kc(kc, [&](auto c) {
        constexpr int KC = decltype(c)::value;
        hd_launch<hmm_hsmm_kernel<KC, LC>, KC>(p, grid, st);
    });
}

extern "C" int abnu_hmm_hsmm_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                                     const float* shift, const float* A, const float* B, const float* c0,
                                     const float* li, const float* lx, int64_t K,
                                     int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                                     void* ws, int64_t ws_bytes, void* stream, const float* ld, const float* ls, int32_t L)
{
    const char* what = "abnu_hmm_hsmm_viterbi";
    const auto check_L = [&]() -> int {
        ABN_REQUIRE(ld && ls, "%s: null pointer", what);
        return hs_check_L(what, L);
    };
    HmmDenseVitP v;                                           // the decoders' prologue fills this; the kernel takes its own flat HsmmP
    int grid;
    const int rc = hd_decode_setup(what, "abnu_hmm_hsmm_viterbi_ws_bytes", check_L, hd_frame_bytes(K, 2, true), x, T, D, off, len, n_utt,
                                   shift, A, B, c0, li, lx, K, ids, log_prob, n_switch, n_good, ws, ws_bytes, &v, &grid);
    if (rc != ABN_OK) return rc;
    HsmmP p;
    p.g = v.g; p.li = v.li; p.lx = v.lt; p.ld = ld; p.ls = ls; p.off = v.off; p.len = v.len; p.n_utt = v.n_utt; p.L = (int)L;
    p.ids = v.ids; p.log_prob = v.log_prob; p.n_switch = v.n_switch; p.n_good = v.n_good;
    p.ws = v.ws; p.per_wg = v.per_wg; p.ks = v.ks; p.cap = v.cap;
    const int kc = hd_kc_for(K);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (L <= 8) hs_launch<8>(p, kc, grid, st);
    else if (L <= 16) hs_launch<16>(p, kc, grid, st);
    else hs_launch<32>(p, kc, grid, st);
    ABN_CHECK_LAUNCH(what);
    return ABN_OK;
}

extern "C" int abnu_hmm_run_stats(const int32_t* ids, int64_t T, const int64_t* off, const int32_t* len, int64_t n_utt, int64_t K,
                                  int32_t L, int64_t* dur, int64_t* tail, void* stream)
{
    const char* what = "abnu_hmm_run_stats";
    ABN_REQUIRE(T >= 1 && T < (1LL << 31), "%s: T = %lld out of range", what, (long long)T);
    ABN_REQUIRE(n_utt >= 1 && n_utt < (1LL << 31), "%s: n_utt = %lld out of range", what, (long long)n_utt);
    ABN_REQUIRE(K >= 1, "%s: K = %lld out of range", what, (long long)K);
    if (K > HD_MAX_K) {
        set_error("%s: K = %lld, supported K <= %d (abny_hmm_dense_max_k)", what, (long long)K, HD_MAX_K);
        return ABN_E_UNSUPPORTED;
    }
    ABN_REQUIRE(ids && off && len && dur && tail, "%s: null pointer", what);
    const int rc = hs_check_L(what, L);
    if (rc != ABN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(dur, 0, (size_t)K * (size_t)L * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(tail, 0, (size_t)K * sizeof(int64_t), st) != hipSuccess) {
        set_error("%s: memset failed", what);
        return ABN_E_LAUNCH;
    }
    HsRunP p;
    p.ids = ids; p.off = off; p.len = len; p.T = T;
    p.K = (int)K; p.L = (int)L; p.n_utt = (int)n_utt;
    p.dur = reinterpret_cast<unsigned long long*>(dur); p.tail = reinterpret_cast<unsigned long long*>(tail);
    const int64_t want = (n_utt + 3) / 4;
    const dim3 grid((unsigned)(want < HS_RUN_GRID ? want : HS_RUN_GRID));
    hipLaunchKernelGGL(hs_run_kernel, grid, dim3(256), hs_run_lds(K, L), st, p);
    ABN_CHECK_LAUNCH(what);
    return ABN_OK;
}
