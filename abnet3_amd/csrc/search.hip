// search.hip -- subsequence DTW for query-by-example search (abnet3_amd/qbe.py): a query Q of M frames is aligned with
// any contiguous run of an utterance U of N frames.  The definition (cells, recurrence, result) is qbe.py's module
// docstring; tests/qbe_np.py restates it in numpy.
//
// dtw_search_kernel (abn_dtw_search_batched, abn_dtw_search_kl_batched) has the shape of abx.hip's dtw_cost_kernel:
// one wavefront per pair (a grid-stride loop over a device-resident pair table); the UTTERANCE is cut into bands of 64
// rows, one per lane, and is unbounded; a band into rounds of 64 anti-diagonals whose cells are first computed
// cell-parallel in 2 x 2 tiles (dtw_tiles.h) into a diagonal-major LDS ring and then swept, the row above arriving over
// a DPP wave shift.  The QUERY is the column side: the band's last row goes to the next band through LDS, which caps
// the query at ABN_DTW_SEARCH_MAX_QUERY frames.  What differs from the ABX kernel:
//   - the free start: in query column 0 the diagonal predecessor of EVERY row i is a virtual cell of cost 0, length 0
//     and start i (and there is no left predecessor); the start index is carried along the chosen predecessor like the
//     length, so the sweep shifts three values and the boundary row holds three;
//   - no pair is dropped: a NaN cosine cell is 0 or 1 when it is a rounding of |cos| above 1 and blocked (+inf)
//     otherwise, a KL cell on a BAD row is blocked; a blocked cell's cost is +inf and paths go round it;
//   - the free end: a lane that leaves the last column keeps (cost, length, start) of its row; after each band a wave
//     reduction of (cost / length, row) is merged into the running best with a strict <, so the first row wins ties;
//   - the optional profile: the lanes write what they kept, per utterance frame.
// LDS per wavefront: ring 16 KiB + boundary row (8 + 4 + 4) x 256 = 4 KiB + query norms 1 KiB + band norms 256 B
// = 21.25 KiB, seven wavefronts to a CU's 160 KiB -- the ABX kernel's count (20.25 KiB).
#include "common.h"
#include "dist_ref.h"
#include "dtw_tiles.h"

namespace abn {
namespace {

constexpr int CB = 64;                              // rows of a band = lanes
constexpr int RD = 64;                              // anti-diagonals of a round (the LDS ring's rows)
constexpr int MAXQ = ABN_DTW_SEARCH_MAX_QUERY;      // query frames a pair may have (the LDS boundary row)

template <bool KL>
struct search_extra {};
template <>
struct search_extra<true> {
    const float* LU;
    const float* LQ;
    const uint8_t* bad_u;
    const uint8_t* bad_q;
};
constexpr bool CELL_COSINE = false, CELL_KL = true;

struct search_out {
    double* total_cost;
    int32_t* path_len;
    int32_t* start;
    int32_t* end;
    const int64_t* prof_off;        // the profile: pair p's utterance frame i is entry prof_off[p] + i (prof_cost == nullptr: none)
    int64_t prof_rows;
    double* prof_cost;
    int32_t* prof_len;
    int32_t* prof_start;
};

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) < __builtin_inff(); }

template <bool VEC, bool KL>
__global__ __launch_bounds__(64) void dtw_search_kernel(const float* __restrict__ utt, int64_t urows,
                                                        const float* __restrict__ qry, int64_t qrows,
                                                        const int64_t* __restrict__ uoff, const int32_t* __restrict__ un,
                                                        const int64_t* __restrict__ qoff, const int32_t* __restrict__ qn,
                                                        int64_t npairs, int D, search_out out, search_extra<KL> ex)
{
    __shared__ float ring[RD][CB];              // [diagonal % RD][row of the band]
    __shared__ double bnd_c[MAXQ];              // the band's last row: costs ...
    __shared__ int32_t bnd_l[MAXQ];             // ... path lengths ...
    __shared__ int32_t bnd_s[MAXQ];             // ... and start rows, per query column
    __shared__ float ny_s[MAXQ];                // cosine: the query frames' norms; KL: 1 for a BAD row, else 0
    __shared__ float nx_s[CB];                  // the same of the band's utterance frames
    const int lane = threadIdx.x;
    const double INF = __builtin_inf();
    const bool prof = out.prof_cost != nullptr;

    for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int64_t o1 = uoff[p], o2 = qoff[p];
        const int N = un[p], M = qn[p];
        bool refused = N < 0 || M < 0 || M > MAXQ || o1 < 0 || o2 < 0 || o1 > urows - N || o2 > qrows - M;
        int64_t po = 0;
        if (!refused && prof) {
            po = out.prof_off[p];
            refused = po < 0 || po > out.prof_rows - N;
        }
        if (refused || N == 0 || M == 0) {                      // refused: nothing is read, no profile entry is written
            if (lane == 0) {
                out.path_len[p] = refused ? -1 : 0;
                out.total_cost[p] = 0.0;
                out.start[p] = -1;
                out.end[p] = -1;
            }
            if (!refused && prof)                               // an empty query: no row has an end
                for (int i = lane; i < N; i += CB) { out.prof_cost[po + i] = INF; out.prof_len[po + i] = 0; out.prof_start[po + i] = -1; }
            continue;
        }
        const float* X = utt + o1 * D;
        const float* Y = qry + o2 * D;
        const float* LX = nullptr;
        const float* LY = nullptr;
        if constexpr (KL) {
            LX = ex.LU + o1 * D;
            LY = ex.LQ + o2 * D;
            for (int j = lane; j < M; j += CB) ny_s[j] = ex.bad_q[o2 + j] != 0 ? 1.0f : 0.0f;
        } else {
            for (int j = lane; j < M; j += CB) ny_s[j] = row_norm_numpy(Y + (int64_t)j * D, D);
        }
        // the running best over the bands done so far (the same in every lane)
        double best_sc = INF, best_c = 0.0;
        int best_l = 0, best_s = -1, best_e = -1;
        for (int i0 = 0; i0 < N; i0 += CB) {
            const int nr = min(CB, N - i0);
            const bool feed = i0 + CB < N;                      // the last row goes to the band below
            if (lane < nr) {
                if constexpr (KL) nx_s[lane] = ex.bad_u[o1 + i0 + lane] != 0 ? 1.0f : 0.0f;
                else nx_s[lane] = row_norm_numpy(X + (int64_t)(i0 + lane) * D, D);
            }
            wave_lds_sync();
            // sweep state of row i0 + lane: (p1, l1, s1) = its cell at the previous column, (up_prev, ...) = the row
            // above one column back (= the diagonal neighbour of the next step)
            double p1 = INF, up_prev = INF;
            int l1 = 0, lup_prev = 0, s1 = -1, sup_prev = -1;
            double fc = INF;                                    // the row's cell in the last query column
            int fl = 0, fs = -1;
            const int ndiag = nr + M - 1;
            for (int s0 = 0; s0 < ndiag; s0 += RD) {
                // ---- produce: the cells (i, j) of band rows with s0 <= i + j < s0 + RD, in 2 x 2 tiles (an odd last
                // row / column repeats its neighbour: the repeated cell is computed and stored twice, the same value)
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
                        const float nx = nx_s[il], ny = ny_s[j];
                        float d;
                        if constexpr (KL) {
                            d = 0.5f * dot[c];
                            if (nx != 0.0f || ny != 0.0f || !(d >= 0.0f)) d = __builtin_inff();     // a BAD row: blocked
                        } else {
                            d = (norm_is_plain(nx) && norm_is_plain(ny)) ? angular_distance_ref<true>(dot[c], nx, ny)
                                                                         : angular_distance_ref<false>(dot[c], nx, ny);
                            if (!(d >= 0.0f)) {
                                // NaN.  With a finite dot product and a finite non-zero product of the norms it is
                                // |cos| rounded above 1: parallel frames (0) or opposite ones (1).  Else: blocked.
                                const float pr = nx * ny;
                                const bool rounding = finite_f32(dot[c]) && finite_f32(pr) && pr != 0.0f;
                                d = rounding ? (dot[c] > 0.0f ? 0.0f : 1.0f) : __builtin_inff();
                            }
                        }
                        ring[s & (RD - 1)][il] = d;
                    }
                }
                wave_lds_sync();
                // ---- sweep: diagonals s0 .. s0 + RD - 1; lane i is at column s - i
                // (the step's LDS operands are read one step ahead: they do not depend on the chain)
                const int ns = min(RD, ndiag - s0);
                float dnext = ring[s0 & (RD - 1)][lane];
                double tnext = INF;
                int tlnext = 0, tsnext = -1;
                if (lane == 0 && i0 > 0 && s0 < M) { tnext = bnd_c[s0]; tlnext = bnd_l[s0]; tsnext = bnd_s[s0]; }
                for (int e = 0; e < ns; ++e) {
                    const int s = s0 + e, j = s - lane;
                    const float dist = dnext;
                    double up = shr1_f64(p1);
                    int lup = shr1_i32(l1), sup = shr1_i32(s1);
                    if (lane == 0) { up = tnext; lup = tlnext; sup = tsnext; }
                    dnext = ring[(s + 1) & (RD - 1)][lane];
                    if (lane == 0 && i0 > 0 && s + 1 < M) { tnext = bnd_c[s + 1]; tlnext = bnd_l[s + 1]; tsnext = bnd_s[s + 1]; }
                    double dg = up_prev;
                    int ldg = lup_prev, sdg = sup_prev;
                    const double left = p1;                     // (column 0: still +inf, there is no left predecessor)
                    up_prev = up;
                    lup_prev = lup;
                    sup_prev = sup;
                    if (lane < nr && (unsigned)j < (unsigned)M) {
                        if (j == 0) { dg = 0.0; ldg = 0; sdg = i0 + lane; }      // the free start: the virtual cell (i - 1, -1)
                        const bool take_up = up < dg;               // first minimum in the order diag, up, left
                        const double b1 = take_up ? up : dg;
                        const bool take_left = left < b1;
                        const double best = take_left ? left : b1;
                        const int lbest = take_left ? l1 : (take_up ? lup : ldg);
                        const int sbest = take_left ? s1 : (take_up ? sup : sdg);
                        p1 = (double)dist + best;
                        l1 = lbest + 1;
                        s1 = sbest;
                        if (feed && lane == CB - 1) { bnd_c[j] = p1; bnd_l[j] = l1; bnd_s[j] = s1; }
                        if (j == M - 1) { fc = p1; fl = l1; fs = s1; }
                    }
                }
                wave_lds_sync();                                // the next round's cells overwrite the ring
            }
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
            if (sc < best_sc) {                                 // strict: an earlier band's row wins a tie
                best_sc = sc;
                best_c = wc;
                best_l = wl;
                best_s = ws;
                best_e = i0 + row;
            }
        }
        if (lane == 0) {
            out.total_cost[p] = best_c;
            out.path_len[p] = best_l;
            out.start[p] = best_s;
            out.end[p] = best_e;
        }
        wave_lds_sync();                                        // ny_s / nx_s / the boundary row: the next pair's
    }
}

bool check_search_args(const char* what, int64_t rows_u, int64_t rows_q, int64_t npairs, int64_t D, const void* tables_ok,
                       const int64_t* u_off, const int32_t* u_n, const int64_t* q_off, const int32_t* q_n,
                       const search_out& o)
{
    if (!(npairs >= 0 && D >= 1 && D < (1 << 20) && rows_u >= 0 && rows_q >= 0)) { set_error("%s: bad npairs/D/rows", what); return false; }
    if (npairs == 0) return true;
    if (!(tables_ok && u_off && u_n && q_off && q_n && o.total_cost && o.path_len && o.start && o.end)) { set_error("%s: null pointer", what); return false; }
    if (o.prof_cost && !(o.prof_off && o.prof_len && o.prof_start && o.prof_rows >= 0)) { set_error("%s: an incomplete profile", what); return false; }
    if (!(rows_u * D < (1LL << 62) && rows_q * D < (1LL << 62))) { set_error("%s: feature array too large", what); return false; }
    return true;
}

}  // namespace
}  // namespace abn

using namespace abn;

extern "C" int64_t abn_dtw_search_max_query(void) { return MAXQ; }

extern "C" int abn_dtw_search_batched(const float* utt, int64_t rows_u, const float* qry, int64_t rows_q,
                                      const int64_t* u_off, const int32_t* u_n, const int64_t* q_off, const int32_t* q_n,
                                      int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, int32_t* start,
                                      int32_t* end, const int64_t* prof_off, int64_t prof_rows, double* prof_cost,
                                      int32_t* prof_len, int32_t* prof_start, void* stream)
{
    const search_out o = {total_cost, path_len, start, end, prof_off, prof_rows, prof_cost, prof_len, prof_start};
    if (!check_search_args("dtw_search", rows_u, rows_q, npairs, D, (utt && qry) ? utt : nullptr, u_off, u_n, q_off, q_n, o))
        return ABN_E_ARG;
    if (npairs == 0) return ABN_OK;
    const int64_t grid = npairs < 256 * 32 ? npairs : 256 * 32;
    const bool vec = D % 4 == 0 && aligned16(utt) && aligned16(qry);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((dtw_search_kernel<true, CELL_COSINE>), dim3((unsigned)grid), dim3(64), 0, st, utt, rows_u, qry, rows_q,
                                u_off, u_n, q_off, q_n, npairs, (int)D, o, search_extra<CELL_COSINE>());
    else hipLaunchKernelGGL((dtw_search_kernel<false, CELL_COSINE>), dim3((unsigned)grid), dim3(64), 0, st, utt, rows_u, qry, rows_q,
                            u_off, u_n, q_off, q_n, npairs, (int)D, o, search_extra<CELL_COSINE>());
    ABN_CHECK_LAUNCH("dtw_search");
    return ABN_OK;
}

extern "C" int abn_dtw_search_kl_batched(const float* PU, const float* LU, int64_t rows_u, const float* PQ, const float* LQ,
                                         int64_t rows_q, const int64_t* u_off, const int32_t* u_n, const int64_t* q_off,
                                         const int32_t* q_n, int64_t npairs, int64_t D, const uint8_t* bad_u,
                                         const uint8_t* bad_q, double* total_cost, int32_t* path_len, int32_t* start,
                                         int32_t* end, const int64_t* prof_off, int64_t prof_rows, double* prof_cost,
                                         int32_t* prof_len, int32_t* prof_start, void* stream)
{
    const search_out o = {total_cost, path_len, start, end, prof_off, prof_rows, prof_cost, prof_len, prof_start};
    if (!check_search_args("dtw_search_kl", rows_u, rows_q, npairs, D, (PU && LU && PQ && LQ && bad_u && bad_q) ? PU : nullptr,
                           u_off, u_n, q_off, q_n, o))
        return ABN_E_ARG;
    if (npairs == 0) return ABN_OK;
    const int64_t grid = npairs < 256 * 32 ? npairs : 256 * 32;
    const bool vec = D % 4 == 0 && aligned16(PU) && aligned16(LU) && aligned16(PQ) && aligned16(LQ);
    hipStream_t st = (hipStream_t)stream;
    const search_extra<CELL_KL> ex = {LU, LQ, bad_u, bad_q};
    if (vec) hipLaunchKernelGGL((dtw_search_kernel<true, CELL_KL>), dim3((unsigned)grid), dim3(64), 0, st, PU, rows_u, PQ, rows_q,
                                u_off, u_n, q_off, q_n, npairs, (int)D, o, ex);
    else hipLaunchKernelGGL((dtw_search_kernel<false, CELL_KL>), dim3((unsigned)grid), dim3(64), 0, st, PU, rows_u, PQ, rows_q,
                            u_off, u_n, q_off, q_n, npairs, (int)D, o, ex);
    ABN_CHECK_LAUNCH("dtw_search_kl");
    return ABN_OK;
}
