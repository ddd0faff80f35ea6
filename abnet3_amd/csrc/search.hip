// search.hip -- subsequence DTW for query-by-example search (abnet3_amd/qbe.py): a query Q of M frames is aligned with
// any contiguous run of an utterance U of N frames.  The definition (cells, recurrence, result) is qbe.py's module
// docstring; tests/qbe_np.py restates it in numpy.
//
// abn_dtw_search_batched and abn_dtw_search_kl_batched are the SEARCH mode of dtw_wave.h's dtw_wave_kernel -- the body
// abx.hip's cost entries run in COST mode; the free start, the blocked cells, the free end and the profile are described
// there.  The UTTERANCE is side 1 (bands of 64 rows, one per lane, unbounded), the QUERY the column side: the band's last
// row goes to the next band through LDS, which caps the query at ABN_DTW_SEARCH_MAX_QUERY frames.
// LDS per wavefront: ring 16 KiB + boundary row (8 + 4 + 4) x 256 = 4 KiB + query norms 1 KiB + band norms 256 B
// = 21.25 KiB, seven wavefronts to a CU's 160 KiB -- the cost mode's count (20.25 KiB; 19 KiB without norms under KL).
#include "dtw_wave.h"

using namespace abn;

extern "C" int64_t abn_dtw_search_max_query(void) { return ABN_DTW_SEARCH_MAX_QUERY; }

extern "C" int abn_dtw_search_batched(const float* utt, int64_t rows_u, const float* qry, int64_t rows_q,
                                      const int64_t* u_off, const int32_t* u_n, const int64_t* q_off, const int32_t* q_n,
                                      int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, int32_t* start,
                                      int32_t* end, const int64_t* prof_off, int64_t prof_rows, double* prof_cost,
                                      int32_t* prof_len, int32_t* prof_start, void* stream)
{
    const dtw_out<MODE_SEARCH> o = {total_cost, path_len, start, end, prof_off, prof_rows, prof_cost, prof_len, prof_start};
    return launch_dtw_wave("dtw_search", utt, rows_u, qry, rows_q, u_off, u_n, q_off, q_n, npairs, D, o,
                           cell_extra<CELL_COSINE>(), stream);
}

extern "C" int abn_dtw_search_kl_batched(const float* PU, const float* LU, int64_t rows_u, const float* PQ, const float* LQ,
                                         int64_t rows_q, const int64_t* u_off, const int32_t* u_n, const int64_t* q_off,
                                         const int32_t* q_n, int64_t npairs, int64_t D, const uint8_t* bad_u,
                                         const uint8_t* bad_q, double* total_cost, int32_t* path_len, int32_t* start,
                                         int32_t* end, const int64_t* prof_off, int64_t prof_rows, double* prof_cost,
                                         int32_t* prof_len, int32_t* prof_start, void* stream)
{
    const dtw_out<MODE_SEARCH> o = {total_cost, path_len, start, end, prof_off, prof_rows, prof_cost, prof_len, prof_start};
    return launch_dtw_wave("dtw_search_kl", PU, rows_u, PQ, rows_q, u_off, u_n, q_off, q_n, npairs, D, o,
                           cell_extra<CELL_KL>{LU, LQ, bad_u, bad_q}, stream);
}
