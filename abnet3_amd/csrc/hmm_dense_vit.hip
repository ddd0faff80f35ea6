// hmm_dense_vit.hip -- the max-product path of the HMM with a full K x K transition matrix (abnz_hmm_dense_viterbi).
// abnet3_amd/hmm.py states the definition, tests/hmm_dense_vit_np.py restates it; DESIGN.md section 3.4c7 the shape.  Behind
// it the same path with a minimum unit duration (hmm_dense_dur_kernel: abnw_hmm_dense_viterbi_dur).  The launch shape, the
// score block, the matrix load, the refusal, the id and result writes and the host side are hmm_dense.h's, described there;
// workspace geometry and checks are utt_chain.h's.  The entry maximum, the key reduction and the plane copies stand in
// both kernels' own text: as shared functions they measured 1 % slower in each kernel at one capacity (the figures are
// beside the text).
//
// hmm_dense_vit_kernel: one sequential step per good frame over the log transitions in LDS (-inf past K).  What the sticky
// decoders (hmm.hip) cannot do and this kernel does:
//   * a true argmax over j for every (frame, k): thread t has own = t % KC (k) and the slice sl = t / KC of SW = KC^2 / 256
//     consecutive j; it takes the max of W[j] + lt[j][own] over its slice with a strict compare in ascending j (the lowest
//     j on ties), the NS = 256 / KC partial (value, j) pairs go through LDS and the threads t < KC combine them slice 0
//     first, again strictly: the lowest j of the maximum, and its value.
//   * W is not stored: the previous frame's u[j] stays in LDS and every reader takes W[j] = u[j] - M itself, M in a
//     register, which saves the frame a third barrier.  u is kept by parity, so a frame has two barriers: behind the
//     partial pairs and behind the wave keys.
//   * M and its lowest index -- at the last good frame the final state -- are ONE 64-bit key max-reduction (vit_wave.h).
//   * a backpointer byte per (frame, k): one plane.  A BAD frame is marked by 0xFF in its first byte (j < 128); the first
//     good frame's bytes are bp[k] = k, so the walk counts no switch there.
// Padding never wins: lt is -inf outside K x K and u is -inf past K (written once, never by an owner), so a padded
// candidate is -inf + -inf = -inf and loses every strict compare against slice 0's j = 0; threads with own >= K put no
// key into the reduction (0 is below every key of a float).  No floating-point atomic, fixed orders throughout; nothing of
// an utterance's results depends on the grid or on its neighbours.
#include "hmm_dense.h"
#include "../../include/abnet3_hip_next.h"

namespace abn {

constexpr unsigned char HDV_BAD = 0xFF;    // a BAD frame's first backpointer byte (every real one is below HD_MAX_K)
static_assert(HD_MAX_K <= 128, "a backpointer is one byte and 0xFF marks a BAD frame");
static_assert((size_t)GM_B * HD_MAX_K <= GM_TILE_BYTES, "a block's backpointers fit over the operand tiles");

template <int KC>
__global__ __launch_bounds__(256) void hmm_dense_vit_kernel(HmmDenseVitP p)
{
    static_assert(256 % KC == 0 && KC * KC % 256 == 0, "256 threads cover KC x KC in slices");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int bad_s[GM_B];
    __shared__ int ids_s[GM_B];
    __shared__ unsigned long long red_k[2][4];
    __shared__ float part_v[256];                                     // [slice][own]
    __shared__ int part_j[256];
    __shared__ float u_s[2][KC];                                      // the previous good frame's u, by parity; -inf past K

    float* const lt_s = smem + 4 * GmTile::floats;                    // [KC][KC + 1], behind the operand tiles
    unsigned char* const bp_s = reinterpret_cast<unsigned char*>(smem);      // [128][KC], over the operand tiles
    const int t = threadIdx.x;
    const int K = p.g.K, ks = p.ks;
    const bool owner = t < K;                                         // state t's chain value is formed by this thread
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = reinterpret_cast<float*>(base);
    unsigned char* const bpw = reinterpret_cast<unsigned char*>(base + (int64_t)sizeof(float) * GM_B * ks);

    hd_load_matrix<KC>(lt_s, p.lt, K, -INFINITY, false);
    if (t < KC) { u_s[0][t] = -INFINITY; u_s[1][t] = -INFINITY; }
    const float li = owner ? p.li[t] : 0.0f;
    __syncthreads();

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (hd_refused(p, u, o, L)) continue;                         // (uniform)
        bool started = false;
        int par = 0, ngood = 0, jlast = -1;
        float M = 0.0f;                                               // the previous good frame's max
        double lp = 0.0;
        const int nblk = (L + GM_B - 1) / GM_B;

        for (int b = 0; b < nblk; ++b) {
            const int f0 = b * GM_B;
            const int nf = min(GM_B, L - f0);
            hd_logn_block(p.g, (int)o + f0, nf, smem, slab, ks, bad_s);

            float sn = owner ? slab[t] : 0.0f;
            for (int f = 0; f < nf; ++f) {
                const float s = sn;
                if (f + 1 < nf) sn = owner ? slab[(int64_t)(f + 1) * ks + t] : 0.0f;
                if (bad_s[f]) {                                       // (uniform) the chain passes over it
                    if (t == 0) bp_s[f * KC] = HDV_BAD;
                    continue;
                }
                float c = li;
                int bj = t;                                           // the first good frame: bp[k] = k
                // (uniform) c[own] = max_j (u[j] - M) + lt[j][own].  This step and the key reduction below are the same text in
                // hmm_dense_dur_kernel, on purpose: as two shared __forceinline__ functions this kernel measured 1.009 to 1.010 x
                // the build without them at (D, K) = (40, 128) (16.21 -> 16.37 ms, run-to-run band 0.1 %), with both in its own
                // text 1.000 to 1.003 x (profiles/hmm_dense_shared_layer.md)
                if (started) {
                    constexpr int NS = 256 / KC, SW = KC / NS, TS = KC + 1;
                    const int own = t % KC, sl = t / KC;
                    const float* const ltc = lt_s + (sl * SW) * TS + own;
                    const float* const uv = u_s[par] + sl * SW;
                    float best = (uv[0] - M) + ltc[0];
                    int bc = 0;
#pragma unroll
                    for (int q = 1; q < SW; ++q) {
                        const float v = (uv[q] - M) + ltc[q * TS];
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
                const float uu = s + c;
                unsigned long long key = 0;                           // (below the key of -inf: the padding never wins)
                if (owner) {
                    u_s[par ^ 1][t] = uu;
                    bp_s[f * KC + t] = (unsigned char)bj;
                    key = vit_key(uu, t);
                }
                {                                                     // the key's max over the workgroup, in every thread
                    const int lane = t & 63, wave = t >> 6;
                    key = vit_wave_max(key);
                    if (lane == 0) red_k[par][wave] = key;
                    __syncthreads();
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned long long ok = red_k[par][w];
                        key = ok > key ? ok : key;
                    }
                }
                M = vit_key_score(key);
                jlast = hd_key_index(key, K);
                lp += (double)M;
                par ^= 1;                                             // (the other sets are not rewritten before the next barrier)
                started = true;
                ++ngood;
            }
            __syncthreads();                                          // the block's backpointers are complete; the slab's readers are done
            if (b + 1 < nblk) {                                       // (uniform; nf == 128) the last block stays in LDS
                const unsigned* const src = reinterpret_cast<const unsigned*>(bp_s);
                unsigned* const dst = reinterpret_cast<unsigned*>(bpw + (int64_t)f0 * KC);
                for (int i = t; i < GM_B * KC / 4; i += 256) dst[i] = src[i];
                __syncthreads();                                      // before the next block's operands replace them
            }
        }

        // The traceback, last block first: jlast is the final state.  cur and nsw live in thread 0.
        // (HDV_NO_TRACEBACK: a timing-only variant without it -- tools/variants.sh, tools/hmm_dense_decode_time.py; ids stay
        // unwritten and n_switch 0.  Never defined in the library's build.)
        int cur = ngood > 0 ? jlast : -1, nsw = 0;
#ifndef HDV_NO_TRACEBACK
        for (int b = nblk - 1; b >= 0; --b) {
            const int f0 = b * GM_B;
            const int nf = min(GM_B, L - f0);
            if (b + 1 < nblk) {                                       // (uniform; nf == 128)
                const unsigned* const src = reinterpret_cast<const unsigned*>(bpw + (int64_t)f0 * KC);
                unsigned* const dst = reinterpret_cast<unsigned*>(bp_s);
                for (int i = t; i < GM_B * KC / 4; i += 256) dst[i] = src[i];
                __syncthreads();
            }
            if (t == 0) {
                for (int f = nf - 1; f >= 0; --f) {
                    const unsigned char* const row = bp_s + f * KC;
                    if (row[0] == HDV_BAD || cur < 0) {
                        ids_s[f] = -1;
                        continue;
                    }
                    ids_s[f] = cur;
                    const int pj = row[cur];
                    nsw += pj != cur;
                    cur = pj;
                }
            }
            hd_write_ids(p.ids, o, f0, nf, ids_s);
        }
#else
        (void)cur;
#endif
        hd_write_results(p, u, lp, nsw, ngood);
    }
}

// ---- minimum duration (abnw_hmm_dense_viterbi_dur; tests/hmm_dense_dur_np.py restates it) ---------
// hmm_dense_vit_kernel with every unit a chain of S states (vit_wave.h's vit_dur_step), S >= 2.  What differs:
//   * the diagonal of lt is -inf in LDS -- a unit is entered from a DIFFERENT unit -- and lt[k][k] is the owner's register ls;
//   * the owner of unit k keeps the chain's normalised values V in SC >= S registers (slot SC - S + i is state i); u_s holds
//     the exit states' U[j][S-1], and every reader forms U - N itself, N the previous good frame's maximum over ALL states:
//     the key reduction runs over each owner's chain maximum.  The same two barriers a frame;
//   * a byte per (frame, k) holds the backpointer in bits 0 .. 6 and the exit state's stay bit in bit 7, so every value of a
//     byte is a real one and a BAD frame is marked elsewhere: one byte per frame behind the region's backpointers
//     (slab | [cap][KC] backpointer bytes | [cap] BAD bytes), bad_s for the block in LDS;
//   * the chasing lane carries (cur, ci) -- unit and chain state -- across blocks and BAD frames; the final ci is the largest
//     state of the final unit whose V is 0, which that unit's owner leaves in LDS.
constexpr unsigned char HDD_STAY = 0x80;
static_assert(HD_MAX_K <= HDD_STAY, "a backpointer is seven bits beside the stay bit");

struct HmmDenseDurP { HmmDenseVitP v; int S; };

template <int KC, int SC>
__global__ __launch_bounds__(256) void hmm_dense_dur_kernel(HmmDenseDurP pd)
{
    static_assert(256 % KC == 0 && KC * KC % 256 == 0, "256 threads cover KC x KC in slices");
    static_assert(SC >= 2 && SC <= VIT_DUR_MAX, "the chain of a unit is held in SC registers");
    const HmmDenseVitP& p = pd.v;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int bad_s[GM_B];
    __shared__ int ids_s[GM_B];
    __shared__ unsigned long long red_k[2][4];
    __shared__ float part_v[256];                                     // [slice][own]
    __shared__ int part_j[256];
    __shared__ float u_s[2][KC];                                      // the previous good frame's exit U, by parity; -inf past K
    __shared__ int fin_s;                                             // the final unit's chain state

    float* const lt_s = smem + 4 * GmTile::floats;                    // [KC][KC + 1], behind the operand tiles; the diagonal -inf
    unsigned char* const bp_s = reinterpret_cast<unsigned char*>(smem);      // [128][KC], over the operand tiles
    const int t = threadIdx.x;
    const int K = p.g.K, ks = p.ks, S = pd.S;
    const int e0 = SC - S;                                            // state i lives in slot e0 + i
    const bool owner = t < K;                                         // unit t's chain is kept by this thread
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = reinterpret_cast<float*>(base);
    unsigned char* const bpw = reinterpret_cast<unsigned char*>(base + (int64_t)sizeof(float) * GM_B * ks);
    unsigned char* const badw = bpw + (int64_t)p.cap * KC;

    hd_load_matrix<KC>(lt_s, p.lt, K, -INFINITY, true);
    if (t < KC) { u_s[0][t] = -INFINITY; u_s[1][t] = -INFINITY; }
    const float li = owner ? p.li[t] : 0.0f;
    const float ls = owner ? p.lt[t * K + t] : 0.0f;
    __syncthreads();

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (hd_refused(p, u, o, L)) continue;                         // (uniform)
        bool started = false;
        int par = 0, ngood = 0, jlast = -1;
        float N = 0.0f;                                               // the previous good frame's max over all states
        float V[SC];                                                  // the chain of unit t, normalised
#pragma unroll
        for (int i = 0; i < SC; ++i) V[i] = -INFINITY;
        double lp = 0.0;
        const int nblk = (L + GM_B - 1) / GM_B;

        for (int b = 0; b < nblk; ++b) {
            const int f0 = b * GM_B;
            const int nf = min(GM_B, L - f0);
            hd_logn_block(p.g, (int)o + f0, nf, smem, slab, ks, bad_s);

            float sn = owner ? slab[t] : 0.0f;
            for (int f = 0; f < nf; ++f) {
                const float s = sn;
                if (f + 1 < nf) sn = owner ? slab[(int64_t)(f + 1) * ks + t] : 0.0f;
                if (bad_s[f]) continue;                               // (uniform) the chain passes over it
                float c = li;                                         // what enters state 0
                int bj = t;                                           // the first good frame: bp[k] = k
                // (uniform) c[own] = max_{j != own} (U[j][S-1] - N) + lt[j][own].  This step, the key reduction below and the plane
                // copies are hmm_dense_vit_kernel's text again, on purpose.  Through shared functions <64, 8> measured 1.010 to
                // 1.012 x the build without them (9.80 -> 9.91 ms, band 0.3 %); with one more phase in the kernel's own text each
                // time: the score block 1.010, the plane copies 1.008, this step 1.002 to 1.003, the key reduction 0.998 to
                // 0.999; these three without the score block 0.996 to 0.998, and with the score block in place of the plane
                // copies 1.007 (profiles/hmm_dense_shared_layer.md)
                if (started) {
                    constexpr int NS = 256 / KC, SW = KC / NS, TS = KC + 1;
                    const int own = t % KC, sl = t / KC;
                    const float* const ltc = lt_s + (sl * SW) * TS + own;
                    const float* const uv = u_s[par] + sl * SW;
                    float best = (uv[0] - N) + ltc[0];
                    int bc = 0;
#pragma unroll
                    for (int q = 1; q < SW; ++q) {
                        const float v = (uv[q] - N) + ltc[q * TS];
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
                    const float m = vit_dur_step<SC>(V, s, c, ls, e0, &st);
                    u_s[par ^ 1][t] = V[SC - 1];
                    bp_s[f * KC + t] = (unsigned char)(bj | (st ? HDD_STAY : 0));
                    key = vit_key(m, t);
                }
                {                                                     // the key's max over the workgroup, in every thread
                    const int lane = t & 63, wave = t >> 6;
                    key = vit_wave_max(key);
                    if (lane == 0) red_k[par][wave] = key;
                    __syncthreads();
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned long long ok = red_k[par][w];
                        key = ok > key ? ok : key;
                    }
                }
                N = vit_key_score(key);
                jlast = hd_key_index(key, K);                         // the lowest unit whose chain holds the maximum
#pragma unroll
                for (int i = 0; i < SC; ++i) V[i] = V[i] - N;
                lp += (double)N;
                par ^= 1;                                             // (the other sets are not rewritten before the next barrier)
                started = true;
                ++ngood;
            }
            __syncthreads();                                          // the block's backpointers are complete; the slab's readers are done
            if (b + 1 < nblk) {                                       // (uniform; nf == 128) the last block stays in LDS
                const unsigned* const src = reinterpret_cast<const unsigned*>(bp_s);
                unsigned* const dst = reinterpret_cast<unsigned*>(bpw + (int64_t)f0 * KC);
                for (int i = t; i < GM_B * KC / 4; i += 256) dst[i] = src[i];
                if (t < GM_B) badw[f0 + t] = (unsigned char)bad_s[t];
                __syncthreads();                                      // before the next block's operands replace them
            }
        }

        // The final state: the largest state of unit jlast at 0, from its owner.  Then the traceback, last block first;
        // cur, ci and nsw live in thread 0.
        if (ngood > 0 && t == jlast) {
            int slot = SC - 1;
#pragma unroll
            for (int i = 0; i < SC; ++i) slot = V[i] == 0.0f ? i : slot;
            fin_s = slot - e0;
        }
        __syncthreads();
        int cur = ngood > 0 ? jlast : -1, ci = 0, nsw = 0;
        if (t == 0 && ngood > 0) ci = fin_s;
        for (int b = nblk - 1; b >= 0; --b) {
            const int f0 = b * GM_B;
            const int nf = min(GM_B, L - f0);
            if (b + 1 < nblk) {                                       // (uniform; nf == 128)
                const unsigned* const src = reinterpret_cast<const unsigned*>(bpw + (int64_t)f0 * KC);
                unsigned* const dst = reinterpret_cast<unsigned*>(bp_s);
                for (int i = t; i < GM_B * KC / 4; i += 256) dst[i] = src[i];
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
                    if (ci == S - 1 && (byte & HDD_STAY)) continue;   // the exit state repeats
                    if (ci > 0) { --ci; continue; }                   // inside the forced advance
                    const int pj = byte & (HDD_STAY - 1);             // state 0: entered from pj's exit state
                    nsw += pj != cur;                                 // (the first good frame holds bp[k] = k)
                    cur = pj;
                    ci = S - 1;
                }
            }
            hd_write_ids(p.ids, o, f0, nf, ids_s);
        }
        hd_write_results(p, u, lp, nsw, ngood);
    }
}

}  // namespace abn

using namespace abn;

// (abnw_hmm_dense_viterbi_dur's regions have the BAD byte whatever S is)
extern "C" int64_t abnz_hmm_dense_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D)
{
    return chain_ws_bytes("abnz_hmm_dense_viterbi_ws_bytes", n_utt, max_len, K, D, HD_LIMITS, hd_frame_bytes(K, 1, false), 0);
}

extern "C" int64_t abnw_hmm_dense_viterbi_dur_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D)
{
    return chain_ws_bytes("abnw_hmm_dense_viterbi_dur_ws_bytes", n_utt, max_len, K, D, HD_LIMITS, hd_frame_bytes(K, 1, true), 0);
}

template <int SC>
static void hdd_launch(const HmmDenseDurP& pd, int kc, int grid, hipStream_t st)
{
    hd_for_kc(kc, [&](auto c) {
        constexpr int KC = decltype(c)::value;
        hd_launch<hmm_dense_dur_kernel<KC, SC>, KC>(pd, grid, st);
    });
}

// Both entries: min_duration (null: the entry has none) is checked behind the pointers.  min_duration = 1 launches
// hmm_dense_vit_kernel itself (the wider regions hold its backpointers and a spare byte a frame).
static int hdv_run(const char* what, const char* ws_fn, const int32_t* min_duration,
                   const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                   const float* shift, const float* A, const float* B, const float* c0, const float* li, const float* lt, int64_t K,
                   int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good, void* ws, int64_t ws_bytes, void* stream)
{
    const int S = min_duration ? *min_duration : 1;
    const auto check_S = [&]() -> int {
        ABN_REQUIRE(S >= 1 && S <= VIT_DUR_MAX, "%s: min_duration = %d, 1 .. %d (abnx_viterbi_dur_max)", what, S, VIT_DUR_MAX);
        return ABN_OK;
    };
    HmmDenseDurP pd;
    int grid;
    const int rc = hd_decode_setup(what, ws_fn, check_S, hd_frame_bytes(K, 1, min_duration != nullptr), x, T, D, off, len, n_utt,
                                   shift, A, B, c0, li, lt, K, ids, log_prob, n_switch, n_good, ws, ws_bytes, &pd.v, &grid);
    if (rc != ABN_OK) return rc;
    pd.S = S;
    const int kc = hd_kc_for(K);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (S == 1) hd_for_kc(kc, [&](auto c) {
        constexpr int KC = decltype(c)::value;
        hd_launch<hmm_dense_vit_kernel<KC>, KC>(pd.v, grid, st);
    });
    else if (S == 2) hdd_launch<2>(pd, kc, grid, st);
    else if (S <= 4) hdd_launch<4>(pd, kc, grid, st);
    else hdd_launch<8>(pd, kc, grid, st);
    ABN_CHECK_LAUNCH(what);
    return ABN_OK;
}

extern "C" int abnz_hmm_dense_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                                      const float* shift, const float* A, const float* B, const float* c0,
                                      const float* li, const float* lt, int64_t K,
                                      int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                                      void* ws, int64_t ws_bytes, void* stream)
{
    return hdv_run("abnz_hmm_dense_viterbi", "abnz_hmm_dense_viterbi_ws_bytes", nullptr, x, T, D, off, len, n_utt, shift, A, B, c0, li, lt, K,
                   ids, log_prob, n_switch, n_good, ws, ws_bytes, stream);
}

// abnz_hmm_dense_viterbi with a minimum duration (include/abnet3_hip_next.h).
extern "C" int abnw_hmm_dense_viterbi_dur(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                                          const float* shift, const float* A, const float* B, const float* c0,
                                          const float* li, const float* lt, int64_t K,
                                          int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                                          void* ws, int64_t ws_bytes, void* stream, int32_t min_duration)
{
    return hdv_run("abnw_hmm_dense_viterbi_dur", "abnw_hmm_dense_viterbi_dur_ws_bytes", &min_duration, x, T, D, off, len, n_utt, shift, A, B,
                   c0, li, lt, K, ids, log_prob, n_switch, n_good, ws, ws_bytes, stream);
}
