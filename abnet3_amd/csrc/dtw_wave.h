// dtw_wave.h -- the wavefront-per-pair DTW: ONE kernel body, dtw_wave_kernel<VEC, KL, MODE>, and its host launcher.
// abx.hip instantiates the COST mode (abn_dtw_cost_batched, abn_dtw_cost_kl_batched), search.hip the SEARCH mode
// (abn_dtw_search_batched, abn_dtw_search_kl_batched), local.hip the LOCAL mode (abn_dtw_local_batched,
// abn_dtw_local_kl_batched).  Every translation unit that includes this file is compiled with -ffp-contract=off.
//
// Shared by all modes.  One wavefront per pair (a grid-stride loop over the device-resident pair table).  Side 1 (ABX:
// token 1; search: the utterance) is cut into BANDS of 64 rows, one row per lane, and is unbounded; a band into ROUNDS
// of 64 anti-diagonals.  A round first computes the cells of its 64 diagonals CELL-PARALLEL -- every lane takes 2 x 2
// tiles of the rectangle of rows x columns that holds them (four chains sharing their loads), so a 15 x 15 pair keeps
// all 64 lanes busy instead of 15 -- and drops them into a diagonal-major ring in LDS (ring[(i + j) & 63][i]).  Then
// the lanes sweep the 64 diagonals: lane i holds row i's cell, the row above arrives over a DPP wave shift, the diagonal
// neighbour is the previous step's upper value; cost = d + min(diag, up, left) in float64 with the first minimum in the
// order diag, up, left, and the path length is carried along the predecessor that rule picks.  The band's last row is
// handed to the next band through LDS, which caps side 2 (ABX: token 2; search: the query) at dtw_out<MODE>::CAP
// columns.  Side-2 norms are computed once per pair (LDS), side-1 norms once per band.  Frames are read from L1 / L2:
// no workspace, one launch.
//
// The cell is a template parameter: the angular distance of dist_ref.h (one fmaf chain over k, numpy's norm order, the
// correctly rounded division, glibc's acosf, / float32(pi)) or, KL, the symmetrised Kullback-Leibler divergence over
// the tables of abn_kl_tables: acc = acc + ((P_p[k] - P_q[k]) * (L_p[k] - L_q[k])) in ascending k, every operation
// rounded to float32 on its own, d = 0.5f * acc (every term is >= 0, so d >= 0 and d == 0 for identical frames).
//
// What the modes differ in (if constexpr at each place; a mode's storage and sweep state do not exist in the other):
//   COST    the sweep carries (cost, length); the virtual cell (-1, -1) costs 0; a cosine cell that is not >= 0 drops
//           the pair, a KL pair with a BAD row in either token is dropped before any cell is computed (no norm arrays);
//           the result is lane nr - 1 of the last band.
//   SEARCH  the sweep carries (cost, length, start) and the boundary row holds three; the free start: in column 0 the
//           diagonal predecessor of EVERY row i is a virtual cell of cost 0, length 0 and start i, and there is no left
//           predecessor; no pair is dropped: a NaN cosine cell is 0 or 1 when it is a rounding of |cos| above 1 and
//           blocked (+inf) otherwise, a KL cell on a BAD row (nx_s / ny_s hold the flags) is blocked; the free end: a
//           lane that leaves the last column keeps its row's cell, and after each band a wave reduction of
//           (cost / length, row) is merged into the running best with a strict <, so the first row wins ties; the
//           optional profile: the lanes write what they kept, per row.
//   LOCAL   Smith-Waterman over the similarity theta - d (abnet3_amd/terms.py's module docstring): any stretch of side
//           1 against any stretch of side 2.  The cells are SEARCH's (no pair is dropped, the same blocked cells); the
//           produce phase also blocks the cells of the exclusion band |(off1 + i) - (off2 + j)| < exclude, so the ring
//           holds d or +inf and the SWEEP subtracts: s = (double)theta - (double)d, one float64 subtraction.  The sweep
//           carries (H, length, start row, start column) and the boundary row holds four; a cell outside the matrix is
//           DEAD (H = 0, length 0, start (-1, -1)) instead of +inf; the predecessor is the first MAXIMUM in the order
//           diag, up, left; a cell whose H is not > 0 is dead.  Every lane keeps the best cell of its row as it goes (a
//           new one only on strictly greater H: the first column wins), and after each band a wave reduction of
//           (H, row), the smaller row winning a tie, is merged into the running best with a strict >: the result is
//           the largest H, ties to the smallest row, then the smallest column, whatever the order of execution.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "dist_ref.h"

namespace abn {

// lane l receives lane l-1's value (lane 0: overridden by the caller)
__device__ __forceinline__ double shr1_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);      // wave_shr:1
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int shr1_i32(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

// LDS hand-off inside ONE wavefront: its LDS operations complete in order, so keeping the compiler from moving
// accesses across is all that is needed
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// the four dot products of rows x0, x1 against rows y0, y1, each ONE fmaf chain in k order (what the oracle's loop and
// the MFMA path of abn_dtw_batched compute): a 2 x 2 tile shares its loads, one load per fma instead of two
template <bool VEC>
__device__ __forceinline__ void dot_tile(const float* __restrict__ x0, const float* __restrict__ x1,
                                         const float* __restrict__ y0, const float* __restrict__ y1, int D, float (&acc)[4])
{
    float a00 = 0.0f, a01 = 0.0f, a10 = 0.0f, a11 = 0.0f;
    if (VEC) {
        for (int k = 0; k < D; k += 4) {
            const float4 p = *reinterpret_cast<const float4*>(x0 + k), q = *reinterpret_cast<const float4*>(x1 + k);
            const float4 u = *reinterpret_cast<const float4*>(y0 + k), v = *reinterpret_cast<const float4*>(y1 + k);
            a00 = fmaf(p.x, u.x, a00); a01 = fmaf(p.x, v.x, a01); a10 = fmaf(q.x, u.x, a10); a11 = fmaf(q.x, v.x, a11);
            a00 = fmaf(p.y, u.y, a00); a01 = fmaf(p.y, v.y, a01); a10 = fmaf(q.y, u.y, a10); a11 = fmaf(q.y, v.y, a11);
            a00 = fmaf(p.z, u.z, a00); a01 = fmaf(p.z, v.z, a01); a10 = fmaf(q.z, u.z, a10); a11 = fmaf(q.z, v.z, a11);
            a00 = fmaf(p.w, u.w, a00); a01 = fmaf(p.w, v.w, a01); a10 = fmaf(q.w, u.w, a10); a11 = fmaf(q.w, v.w, a11);
        }
    } else {
        for (int k = 0; k < D; ++k) {
            const float p = x0[k], q = x1[k], u = y0[k], v = y1[k];
            a00 = fmaf(p, u, a00); a01 = fmaf(p, v, a01); a10 = fmaf(q, u, a10); a11 = fmaf(q, v, a11);
        }
    }
    acc[0] = a00; acc[1] = a01; acc[2] = a10; acc[3] = a11;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the four symmetrised-KL sums of rows x0, x1 against rows y0, y1 (P and L tables): per k and cell a subtraction of
// the P's, one of the L's, their product and the addition to the cell's sum, each rounded to float32 (the file is
// compiled without fma contraction).  Two cells to a float2, so the compiler may issue v_pk_add_f32 / v_pk_mul_f32;
// packed or not, every lane of every operation is the IEEE result.  The eight loads of a k step serve four cells.
template <bool VEC>
__device__ __forceinline__ void kl_tile(const float* __restrict__ px0, const float* __restrict__ px1,
                                        const float* __restrict__ lx0, const float* __restrict__ lx1,
                                        const float* __restrict__ py0, const float* __restrict__ py1,
                                        const float* __restrict__ ly0, const float* __restrict__ ly1, int D, float (&acc)[4])
{
    f32x2 a0 = {0.0f, 0.0f}, a1 = {0.0f, 0.0f};        // (a00, a01), (a10, a11)
#define ABN_KL_STEP(P0, P1, L0, L1, PU, PV, LU, LV)                                     \
    do {                                                                                \
        const f32x2 pu_ = {PU, PV}, lu_ = {LU, LV};                                     \
        const f32x2 p0_ = {P0, P0}, l0_ = {L0, L0}, p1_ = {P1, P1}, l1_ = {L1, L1};     \
        a0 = a0 + ((p0_ - pu_) * (l0_ - lu_));                                          \
        a1 = a1 + ((p1_ - pu_) * (l1_ - lu_));                                          \
    } while (0)
    if (VEC) {
        for (int k = 0; k < D; k += 4) {
            const float4 p = *reinterpret_cast<const float4*>(px0 + k), q = *reinterpret_cast<const float4*>(px1 + k);
            const float4 lp = *reinterpret_cast<const float4*>(lx0 + k), lq = *reinterpret_cast<const float4*>(lx1 + k);
            const float4 u = *reinterpret_cast<const float4*>(py0 + k), v = *reinterpret_cast<const float4*>(py1 + k);
            const float4 lu = *reinterpret_cast<const float4*>(ly0 + k), lv = *reinterpret_cast<const float4*>(ly1 + k);
            ABN_KL_STEP(p.x, q.x, lp.x, lq.x, u.x, v.x, lu.x, lv.x);
            ABN_KL_STEP(p.y, q.y, lp.y, lq.y, u.y, v.y, lu.y, lv.y);
            ABN_KL_STEP(p.z, q.z, lp.z, lq.z, u.z, v.z, lu.z, lv.z);
            ABN_KL_STEP(p.w, q.w, lp.w, lq.w, u.w, v.w, lu.w, lv.w);
        }
    } else {
        for (int k = 0; k < D; ++k) ABN_KL_STEP(px0[k], px1[k], lx0[k], lx1[k], py0[k], py1[k], ly0[k], ly1[k]);
    }
#undef ABN_KL_STEP
    acc[0] = a0.x; acc[1] = a0.y; acc[2] = a1.x; acc[3] = a1.y;
}

// what the KL cell reads beside the two P tables (feats1 / feats2 of the kernel); the cosine cell has nothing here
template <bool KL>
struct cell_extra {
    bool complete() const { return true; }
    bool aligned() const { return true; }
};
template <>
struct cell_extra<true> {
    const float* L1;
    const float* L2;
    const uint8_t* bad1;
    const uint8_t* bad2;
    bool complete() const { return L1 && L2 && bad1 && bad2; }
    bool aligned() const { return aligned16(L1) && aligned16(L2); }
};
constexpr bool CELL_COSINE = false, CELL_KL = true;
enum dtw_mode { MODE_COST, MODE_SEARCH, MODE_LOCAL };

// what a mode writes per pair, and the columns it takes (its LDS boundary row); LOCAL: its two parameters ride along
template <dtw_mode MODE>
struct dtw_out;
template <>
struct dtw_out<MODE_COST> {
    static constexpr int CAP = ABN_DTW_COST_MAX_N2;
    double* total_cost;
    int32_t* path_len;
    int parallel_zero;              // cosine cell: != 0 reads a cosine rounded beyond +-1 as distance 0 / 1 (as SEARCH does), 0 drops the pair
    bool complete() const { return total_cost && path_len; }
};
template <>
struct dtw_out<MODE_SEARCH> {
    static constexpr int CAP = ABN_DTW_SEARCH_MAX_QUERY;
    double* total_cost;
    int32_t* path_len;
    int32_t* start;
    int32_t* end;
    const int64_t* prof_off;        // the profile: pair p's row i is entry prof_off[p] + i (prof_cost == nullptr: none)
    int64_t prof_rows;
    double* prof_cost;
    int32_t* prof_len;
    int32_t* prof_start;
    bool complete() const { return total_cost && path_len && start && end; }
};
template <>
struct dtw_out<MODE_LOCAL> {
    static constexpr int CAP = ABN_DTW_LOCAL_MAX_N2;
    double* score;                  // H of the best cell
    int32_t* path_len;
    int32_t* start1;                // the path's first cell (side 1 row, side 2 column) ...
    int32_t* start2;
    int32_t* end1;                  // ... and the best cell itself; stretch-relative, inclusive
    int32_t* end2;
    float theta;                    // similarity = theta - distance
    int64_t exclude;                // > 0: the cells with |(off1 + i) - (off2 + j)| < exclude are blocked
    bool complete() const { return score && path_len && start1 && start2 && end1 && end2; }
};

// what only the LOCAL sweep carries (the other modes' instances are empty, so their code does not change with it):
// per band, beside (p1, l1, s1) = (H, length, start row): the start column of the lane's cell, of the row above one
// column back and of the boundary row's next entry, and the best cell of the lane's row so far
template <bool LOCAL>
struct local_sweep {};
template <>
struct local_sweep<true> {
    int t1 = -1, tup_prev = -1, ttnext = -1;
    double rb_h = 0.0;
    int rb_l = 0, rb_si = -1, rb_sj = -1, rb_j = -1;
};
// ... and per pair: the running best over the bands done so far (the same in every lane; H = 0: no live cell yet)
template <bool LOCAL>
struct local_best {};
template <>
struct local_best<true> {
    double h = 0.0;
    int l = 0, si = -1, sj = -1, ei = -1, ej = -1;
};

namespace {

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) < __builtin_inff(); }

template <bool VEC, bool KL, dtw_mode MODE>
__global__ __launch_bounds__(64) void dtw_wave_kernel(const float* __restrict__ feats1, int64_t rows1,
                                                      const float* __restrict__ feats2, int64_t rows2,
                                                      const int64_t* __restrict__ off1, const int32_t* __restrict__ n1,
                                                      const int64_t* __restrict__ off2, const int32_t* __restrict__ n2,
                                                      int64_t npairs, int D, dtw_out<MODE> out, cell_extra<KL> ex)
{
    constexpr bool SEARCH = MODE == MODE_SEARCH, LOCAL = MODE == MODE_LOCAL;
    constexpr bool FREE = MODE != MODE_COST;    // SEARCH and LOCAL: no pair is dropped, cells are blocked instead
    constexpr int CB = 64;                      // rows of a band = lanes
    constexpr int RD = 64;                      // anti-diagonals of a round (the LDS ring's rows; 32 measured the same)
    constexpr int CAP = dtw_out<MODE>::CAP;
    __shared__ float ring[RD][CB];              // [diagonal % RD][row of the band]
    __shared__ double bnd_c[CAP];               // the band's last row: costs ...
    __shared__ int32_t bnd_l[CAP];              // ... path lengths ...
    __shared__ int32_t bnd_s[CAP];              // ... and (SEARCH, LOCAL) start rows, per column ...
    __shared__ int32_t bnd_t[LOCAL ? CAP : 1];  // ... and (LOCAL) start columns
    __shared__ float ny_s[CAP];                 // cosine: side 2's norms; KL SEARCH / LOCAL: 1 for a BAD row, else 0; KL COST: none
    __shared__ float nx_s[CB];                  // the same of the band's rows
    const int lane = threadIdx.x;
    const double INF = __builtin_inf();
    bool prof = false;
    if constexpr (SEARCH) prof = out.prof_cost != nullptr;

    for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int64_t o1 = off1[p], o2 = off2[p];
        const int N = n1[p], M = n2[p];
        bool refused = N < 0 || M < 0 || M > CAP || o1 < 0 || o2 < 0 || o1 > rows1 - N || o2 > rows2 - M;
        int64_t po = 0;
        if constexpr (SEARCH) {
            if (!refused && prof) {
                po = out.prof_off[p];
                refused = po < 0 || po > out.prof_rows - N;
            }
        }
        if (refused || N == 0 || M == 0) {                      // refused: nothing is read, no profile entry is written
            if (lane == 0) {
                out.path_len[p] = refused ? -1 : 0;
                if constexpr (LOCAL) {
                    out.score[p] = 0.0;
                    out.start1[p] = -1; out.start2[p] = -1; out.end1[p] = -1; out.end2[p] = -1;
                } else {
                    out.total_cost[p] = 0.0;
                }
                if constexpr (SEARCH) { out.start[p] = -1; out.end[p] = -1; }
            }
            if constexpr (SEARCH) {
                if (!refused && prof)                           // an empty query: no row has an end
                    for (int i = lane; i < N; i += CB) { out.prof_cost[po + i] = INF; out.prof_len[po + i] = 0; out.prof_start[po + i] = -1; }
            }
            continue;
        }
        const float* X = feats1 + o1 * D;
        const float* Y = feats2 + o2 * D;
        const float* LX = nullptr;
        const float* LY = nullptr;
        bool bad = false;                                       // COST: the pair is dropped
        if constexpr (KL) {
            LX = ex.L1 + o1 * D;
            LY = ex.L2 + o2 * D;
            if constexpr (FREE) {
                for (int j = lane; j < M; j += CB) ny_s[j] = ex.bad2[o2 + j] != 0 ? 1.0f : 0.0f;
            } else {                                            // a BAD row in either token: dropped before any cell
                for (int i = lane; i < N; i += CB) bad |= ex.bad1[o1 + i] != 0;
                for (int j = lane; j < M; j += CB) bad |= ex.bad2[o2 + j] != 0;
                if (__any(bad)) {
                    if (lane == 0) { out.path_len[p] = 0; out.total_cost[p] = 0.0; }
                    continue;
                }
            }
        } else {
            for (int j = lane; j < M; j += CB) ny_s[j] = row_norm_numpy(Y + (int64_t)j * D, D);
        }
        double fin_c = 0.0;                                     // COST: cell (N - 1, M - 1)
        int fin_l = 0;
        double best_sc = INF, best_c = 0.0;                     // SEARCH: the running best over the bands done so far
        int best_l = 0, best_s = -1, best_e = -1;               // (the same in every lane)
        local_best<LOCAL> lb;                                   // LOCAL: the same
        for (int i0 = 0; i0 < N; i0 += CB) {
            const int nr = min(CB, N - i0);
            const bool feed = i0 + CB < N;                      // the last row goes to the band below
            if constexpr (!KL || FREE) {
                if (lane < nr) {
                    if constexpr (KL) nx_s[lane] = ex.bad1[o1 + i0 + lane] != 0 ? 1.0f : 0.0f;
                    else nx_s[lane] = row_norm_numpy(X + (int64_t)(i0 + lane) * D, D);
                }
                wave_lds_sync();
            }
            // sweep state of row i0 + lane: (p1, l1, s1) = its cell at the previous column, (up_prev, ...) = the row
            // above one column back (= the diagonal neighbour of the next step); COST: the virtual cell (-1, -1) costs 0
            // LOCAL: (p1, l1, s1, ls.t1) = (H, length, start row, start column); outside the matrix: the dead cell
            double p1 = LOCAL ? 0.0 : INF, up_prev = (!SEARCH && i0 == 0 && lane == 0) || LOCAL ? 0.0 : INF;
            int l1 = 0, lup_prev = 0, s1 = -1, sup_prev = -1;
            local_sweep<LOCAL> ls;
            double fc = INF;                                    // SEARCH: the row's cell in the last column
            int fl = 0, fs = -1;
            const int ndiag = nr + M - 1;
            for (int s0 = 0; s0 < ndiag; s0 += RD) {
                // ---- produce: the cells (i, j) of band rows with s0 <= i + j < s0 + RD, in 2 x 2 tiles, one per lane at
                // a time (an odd last row / column repeats its neighbour: the repeated cell is computed and stored twice,
                // the same value)
                const int jlo = max(0, s0 - (nr - 1)), jhi = min(M, s0 + RD);
                const int tr = (nr + 1) >> 1, ntile = tr * ((jhi - jlo + 1) >> 1);
                for (int t = lane; t < ntile; t += CB) {
                    const int tj = t / tr, ia = 2 * (t - tj * tr), ja = jlo + 2 * tj;
                    const int ib = min(ia + 1, nr - 1), jb = min(ja + 1, jhi - 1);
                    float dot[4];
                    const int64_t xa = (int64_t)(i0 + ia) * D, xb = (int64_t)(i0 + ib) * D;
                    const int64_t ya = (int64_t)ja * D, yb = (int64_t)jb * D;
                    if constexpr (KL) kl_tile<VEC>(X + xa, X + xb, LX + xa, LX + xb, Y + ya, Y + yb, LY + ya, LY + yb, D, dot);
                    else dot_tile<VEC>(X + xa, X + xb, Y + ya, Y + yb, D, dot);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int il = c < 2 ? ia : ib, j = (c & 1) ? jb : ja, s = il + j;
                        if (s < s0 || s >= s0 + RD) continue;
                        float d;
                        if constexpr (KL) {
                            d = 0.5f * dot[c];
                            if constexpr (FREE)                     // a BAD row: blocked
                                if (nx_s[il] != 0.0f || ny_s[j] != 0.0f || !(d >= 0.0f)) d = __builtin_inff();
                        } else {
                            const float nx = nx_s[il], ny = ny_s[j];
                            d = (norm_is_plain(nx) && norm_is_plain(ny)) ? angular_distance_ref<true>(dot[c], nx, ny)
                                                                         : angular_distance_ref<false>(dot[c], nx, ny);
                            if constexpr (!FREE) {
                                if (!(d >= 0.0f)) {                 // utils.py:59: the pair is dropped, unless the caller
                                    const float pr = nx * ny;       // asked for the SEARCH rule below and it applies
                                    if (out.parallel_zero && finite_f32(dot[c]) && finite_f32(pr) && pr != 0.0f)
                                        d = dot[c] > 0.0f ? 0.0f : 1.0f;
                                    else bad = true;
                                }
                            } else if (!(d >= 0.0f)) {
                                // NaN.  With a finite dot product and a finite non-zero product of the norms it is
                                // |cos| rounded above 1: parallel frames (0) or opposite ones (1).  Else: blocked.
                                const float pr = nx * ny;
                                const bool rounding = finite_f32(dot[c]) && finite_f32(pr) && pr != 0.0f;
                                d = rounding ? (dot[c] > 0.0f ? 0.0f : 1.0f) : __builtin_inff();
                            }
                        }
                        if constexpr (LOCAL) {                      // the exclusion band, in table rows
                            const int64_t gap = (o1 + i0 + il) - (o2 + j);
                            if ((gap < 0 ? -gap : gap) < out.exclude) d = __builtin_inff();
                        }
                        ring[s & (RD - 1)][il] = d;
                    }
                }
                wave_lds_sync();
                // ---- sweep: diagonals s0 .. s0 + RD - 1; lane i is at column s - i
                // (the step's LDS operands are read one step ahead: they do not depend on the chain)
                const int ns = min(RD, ndiag - s0);
                float dnext = ring[s0 & (RD - 1)][lane];
                double tnext = LOCAL ? 0.0 : INF;
                int tlnext = 0, tsnext = -1;
                if constexpr (LOCAL) ls.ttnext = -1;
                if (lane == 0 && i0 > 0 && s0 < M) {
                    tnext = bnd_c[s0];
                    tlnext = bnd_l[s0];
                    if constexpr (FREE) tsnext = bnd_s[s0];
                    if constexpr (LOCAL) ls.ttnext = bnd_t[s0];
                }
                for (int e = 0; e < ns; ++e) {
                    const int s = s0 + e, j = s - lane;
                    const float dist = dnext;
                    double up = shr1_f64(p1);
                    int lup = shr1_i32(l1), sup = -1;
                    if constexpr (FREE) sup = shr1_i32(s1);
                    if (lane == 0) { up = tnext; lup = tlnext; sup = tsnext; }
                    dnext = ring[(s + 1) & (RD - 1)][lane];
                    if (lane == 0 && i0 > 0 && s + 1 < M) {
                        tnext = bnd_c[s + 1];
                        tlnext = bnd_l[s + 1];
                        if constexpr (FREE) tsnext = bnd_s[s + 1];
                    }
                    double dg = up_prev;
                    int ldg = lup_prev, sdg = sup_prev;
                    const double left = p1;                     // (SEARCH, column 0: still +inf, there is no left predecessor)
                    up_prev = up;
                    lup_prev = lup;
                    sup_prev = sup;
                    if constexpr (LOCAL) {
                        int tup = shr1_i32(ls.t1);                  // (the step's values were fetched above: dist, up, ...)
                        if (lane == 0) tup = ls.ttnext;
                        if (lane == 0 && i0 > 0 && s + 1 < M) ls.ttnext = bnd_t[s + 1];
                        const int tdg = ls.tup_prev;
                        ls.tup_prev = tup;
                        if (lane < nr && (unsigned)j < (unsigned)M) {
                            const bool take_up = up > dg;           // first maximum in the order diag, up, left
                            const double b1 = take_up ? up : dg;
                            const bool take_left = left > b1;
                            const double best = take_left ? left : b1;
                            const int lbest = take_left ? l1 : (take_up ? lup : ldg);
                            const int sbest = take_left ? s1 : (take_up ? sup : sdg);
                            const int tbest = take_left ? ls.t1 : (take_up ? tup : tdg);
                            // a dead predecessor is (0, 0): best + sim is sim and lbest + 1 is 1, the start is the cell's own
                            const bool ext = best > 0.0;
                            const double h = best + ((double)out.theta - (double)dist);
                            const bool live = h > 0.0;
                            p1 = live ? h : 0.0;
                            l1 = live ? lbest + 1 : 0;
                            s1 = live ? (ext ? sbest : i0 + lane) : -1;
                            ls.t1 = live ? (ext ? tbest : j) : -1;
                            if (feed && lane == CB - 1) { bnd_c[j] = p1; bnd_l[j] = l1; bnd_s[j] = s1; bnd_t[j] = ls.t1; }
                            if (p1 > ls.rb_h) {                     // strict: the first column
                                ls.rb_h = p1; ls.rb_l = l1; ls.rb_si = s1; ls.rb_sj = ls.t1; ls.rb_j = j;
                            }
                        }
                    } else if (lane < nr && (unsigned)j < (unsigned)M) {
                        if constexpr (SEARCH)                       // the free start: the virtual cell (i - 1, -1)
                            if (j == 0) { dg = 0.0; ldg = 0; sdg = i0 + lane; }
                        const bool take_up = up < dg;               // first minimum in the order diag, up, left
                        const double b1 = take_up ? up : dg;
                        const bool take_left = left < b1;
                        const double best = take_left ? left : b1;
                        const int lbest = take_left ? l1 : (take_up ? lup : ldg);
                        if constexpr (SEARCH) s1 = take_left ? s1 : (take_up ? sup : sdg);
                        p1 = (double)dist + best;
                        l1 = lbest + 1;
                        if (feed && lane == CB - 1) {
                            bnd_c[j] = p1;
                            bnd_l[j] = l1;
                            if constexpr (SEARCH) bnd_s[j] = s1;
                        }
                        if constexpr (SEARCH)
                            if (j == M - 1) { fc = p1; fl = l1; fs = s1; }
                    }
                }
                wave_lds_sync();                                // the next round's cells overwrite the ring
            }
            if constexpr (LOCAL) {
                // ---- the band's best cell: the largest H, the smaller row on a tie (lanes >= nr hold 0: never taken)
                double h = ls.rb_h;
                int row = lane;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double oh = __shfl_xor(h, o);
                    const int orow = __shfl_xor(row, o);
                    if (oh > h || (oh == h && orow < row)) { h = oh; row = orow; }
                }
                const int wl = __shfl(ls.rb_l, row), wsi = __shfl(ls.rb_si, row), wsj = __shfl(ls.rb_sj, row);
                const int wj = __shfl(ls.rb_j, row);
                if (h > lb.h) {                                 // strict: an earlier band's row wins a tie
                    lb.h = h;
                    lb.l = wl;
                    lb.si = wsi;
                    lb.sj = wsj;
                    lb.ei = i0 + row;
                    lb.ej = wj;
                }
            } else if constexpr (!SEARCH) {
                if (i0 + nr == N) {                             // lane nr - 1 holds cell (N - 1, M - 1)
                    fin_c = __shfl(p1, nr - 1);
                    fin_l = __shfl(l1, nr - 1);
                }
            } else {
                // ---- the band's ends: every lane < nr holds its row's cell of the last column
                const bool fin = lane < nr && fc < INF;
                if (prof && lane < nr) {
                    out.prof_cost[po + i0 + lane] = fin ? fc : INF;
                    out.prof_len[po + i0 + lane] = fin ? fl : 0;
                    out.prof_start[po + i0 + lane] = fin ? fs : -1;
                }
                double sc = fin ? fc / (double)fl : INF;
                int row = lane;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double osc = __shfl_xor(sc, o);
                    const int orow = __shfl_xor(row, o);
                    if (osc < sc || (osc == sc && orow < row)) { sc = osc; row = orow; }
                }
                const double wc = __shfl(fc, row);
                const int wl = __shfl(fl, row), ws = __shfl(fs, row);
                if (sc < best_sc) {                             // strict: an earlier band's row wins a tie
                    best_sc = sc;
                    best_c = wc;
                    best_l = wl;
                    best_s = ws;
                    best_e = i0 + row;
                }
            }
        }
        if constexpr (LOCAL) {
            if (lane == 0) {
                out.score[p] = lb.h;
                out.path_len[p] = lb.l;
                out.start1[p] = lb.si;
                out.start2[p] = lb.sj;
                out.end1[p] = lb.ei;
                out.end2[p] = lb.ej;
            }
        } else if constexpr (!SEARCH) {
            const bool dropped = __any(bad);
            if (lane == 0) {
                out.total_cost[p] = dropped ? 0.0 : fin_c;
                out.path_len[p] = dropped ? 0 : fin_l;
            }
        } else if (lane == 0) {
            out.total_cost[p] = best_c;
            out.path_len[p] = best_l;
            out.start[p] = best_s;
            out.end[p] = best_e;
        }
        wave_lds_sync();                                        // ny_s / nx_s / the boundary row: the next pair's
    }
}

// the host side of every entry point: argument checks (errors are prefixed with `what`), the grid (a wavefront per pair,
// at most 256 * 32 of them), vector loads when every table the cell reads allows them, the launch
template <bool KL, dtw_mode MODE>
int launch_dtw_wave(const char* what, const float* feats1, int64_t rows1, const float* feats2, int64_t rows2,
                    const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int64_t npairs,
                    int64_t D, const dtw_out<MODE>& out, const cell_extra<KL>& ex, void* stream)
{
    ABN_REQUIRE(npairs >= 0 && D >= 1 && D < (1 << 20) && rows1 >= 0 && rows2 >= 0, "%s: bad npairs/D/rows", what);
    if (npairs == 0) return ABN_OK;
    ABN_REQUIRE(feats1 && feats2 && ex.complete() && off1 && n1 && off2 && n2 && out.complete(), "%s: null pointer", what);
    if constexpr (MODE == MODE_SEARCH)
        ABN_REQUIRE(!out.prof_cost || (out.prof_off && out.prof_len && out.prof_start && out.prof_rows >= 0),
                    "%s: an incomplete profile", what);
    ABN_REQUIRE(rows1 * D < (1LL << 62) && rows2 * D < (1LL << 62), "%s: feature array too large", what);
    const int64_t grid = npairs < 256 * 32 ? npairs : 256 * 32;
    const bool vec = D % 4 == 0 && aligned16(feats1) && aligned16(feats2) && ex.aligned();
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((dtw_wave_kernel<true, KL, MODE>), dim3((unsigned)grid), dim3(64), 0, st, feats1, rows1, feats2, rows2,
                                off1, n1, off2, n2, npairs, (int)D, out, ex);
    else hipLaunchKernelGGL((dtw_wave_kernel<false, KL, MODE>), dim3((unsigned)grid), dim3(64), 0, st, feats1, rows1, feats2, rows2,
                            off1, n1, off2, n2, npairs, (int)D, out, ex);
    ABN_CHECK_LAUNCH(what);
    return ABN_OK;
}

}  // namespace
}  // namespace abn
