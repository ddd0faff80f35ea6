"""ctypes binding of libabnet3_hip.so (include/abnet3_hip.h, include/abnet3_hip_next.h).

There is no CPU fallback: if the shared object is missing or a tensor is not
on a HIP device the call fails loudly.  torch is imported first so that the
library binds to the HIP runtime torch already loaded (one runtime instance =
shared streams and allocations).
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL: see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
# ABNET3_HIP_LIB points at another build of the same library (kernel experiments)
LIB_PATH = os.environ.get('ABNET3_HIP_LIB') or os.path.join(HERE, 'lib', 'libabnet3_hip.so')
ABI_VERSION = 20
MAX_LAYERS = 16

ACT = {'none': 0, None: 0, 'sigmoid': 1, 'relu': 2, 'tanh': 3}
LOSS = {'coscos2': 0, 'cosmargin': 1, 'KLLoss': 2}
# abn_pair_loss_dz's "e1 / e2 are the softmax's inputs" (ABN_ACT_SOFTMAX): not in ACT, which the tower
# descriptors read -- no tower kernel takes it
ACT_SOFTMAX = 4
PRECISION = {'fp32': 0, 'bf16': 1, 'bf16x3': 2, 'f16x2': 3}
OPT = {'sgd': 0, 'adadelta': 1, 'adam': 2, 'adagrad': 3, 'RMSprop': 4}
Y_DTYPE = {torch.int8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3,
           torch.float64: 4}

# every symbol include/abnet3_hip.h declares: (restype, argtypes)
_i64, _i32, _f32, _vp = C.c_int64, C.c_int32, C.c_float, C.c_void_p
SYMBOLS = {
    'abn_abi_version': (C.c_int, []),
    'abn_last_error': (C.c_char_p, []),
    'abn_tower_ws_floats': (_i64, [_vp, _i64, _i64]),
    'abn_tower_out_offset': (_i64, [_vp, _i64, _i64]),
    'abn_tower_bwd_scratch_floats': (_i64, [_vp, _i64]),
    'abn_tower_forward': (C.c_int, [_vp, _vp, _vp, _i64, _i64, C.c_int, _vp, _vp]),
    'abn_tower_backward': (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp,
                                      _i64, _vp, _vp]),
    'abn_tower_wpack_floats': (_i64, [_vp]),
    'abn_tower_uses_planes': (C.c_int, [_vp, _i64, _vp, _vp, _vp, C.c_int]),
    'abn_tower_path': (C.c_int, [_vp, _vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _vp]),
    'abn_tower_image_offset': (_i64, [_vp, _i64, _i64, C.c_int, C.c_int]),
    'abn_reload_switches': (None, []),
    'abn_rccl_allreduce_f64': (C.c_int, [_vp, _vp, _i64, _vp]),
    'abn_tower_backward_launch': (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, C.c_int, _vp]),
    'abn_tower_backward_loss_ws_bytes': (_i64, [_i64]),
    'abn_tower_backward_loss': (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, _f32, C.c_int, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    'abn_tower_reduce_step': (C.c_int, [_vp, _i64, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32,
                                         _f32, _i64, _f32, _vp]),
    'abn_linear_forward': (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, C.c_int, _vp, _vp]),
    'abn_linear_dgrad': (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, C.c_int, _vp, _vp]),
    'abn_linear_wgrad_scratch_floats': (_i64, [_i64, _i64, _i64]),
    'abn_linear_wgrad': (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]),
    'abn_linear_backward': (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp, _vp, _i64, _vp]),
    'abn_linear_backward_prec': (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _i64, _vp]),
    'abn_softmax_rows': (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    'abn_softmax_rows_backward': (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    'abn_pair_loss_ws_bytes': (_i64, [_i64]),
    'abn_pair_loss': (C.c_int, [_vp, _vp, _vp, C.c_int, _i64, _i64, C.c_int,
                                 _f32, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'abn_pair_loss_padded': (C.c_int, [_vp, _vp, _vp, C.c_int, _i64, _i64, C.c_int, _f32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'abn_pair_loss_dz': (C.c_int, [_vp, _vp, _vp, C.c_int, _i64, _i64, C.c_int, _f32, C.c_int, C.c_int,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'abn_optimizer_step': (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _i64, _f32,
                                      _f32, _f32, _f32, _i64, _f32, _vp]),
    'abn_tower_sync_ws_bytes': (_i64, []),
    'abn_oneshot_mail_bytes': (_i64, [_i32, _i64]),
    'abn_allreduce_oneshot': (C.c_int, [_vp, _vp, _i64, _vp]),
    'abn_dtw_ws_bytes': (_i64, [_vp, _vp, _i64, _i64, _i64]),
    'abn_dtw_host_stage_bytes': (_i64, [_vp, _vp, _i64]),
    'abn_dtw_batched': (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64,
                                   _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp,
                                   _i64, _vp]),
    'abn_dtw_batched_overlap': (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64,
                                           _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp,
                                           _i64, _vp, _vp]),
    'abn_dtw_cost_max_n2': (_i64, []),
    'abn_dtw_cost_batched': (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    'abn_dtw_cost_parallel_batched': (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    'abn_kl_tables': (C.c_int, [_vp, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    'abn_dtw_cost_kl_batched': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp,
                                           _vp]),
    'abn_abx_score': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    'abn_dtw_search_max_query': (_i64, []),
    'abn_dtw_search_batched': (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp,
                                          _vp, _vp, _vp]),
    'abn_dtw_search_kl_batched': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'abn_dtw_local_max_n2': (_i64, []),
    'abn_dtw_local_batched': (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp]),
    'abn_dtw_local_kl_batched': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _f32, _i64,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'abn_edit_max_short': (_i64, []),
    'abn_edit_distance_batched': (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    'abn_lsh_signatures': (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    'abn_lsh_diag_hits_batched': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                             _vp, _vp, _vp, _vp]),
    'abn_cosine_distance': (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp]),
    'abn_cosine_distance_f64': (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp]),
    'abn_arccos_f32': (C.c_int, [_vp, _i64, C.c_int, _vp, _vp]),
    'abn_gather_rows': (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    'abn_gather_pairs': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    'abn_stack_frames': (C.c_int, [_vp, _i64, _i64, _i32, _vp, _vp]),
    'abn_stack_frames_batched': (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp]),
    'abn_mvn_ws_bytes': (_i64, [_i64, _i64]),
    'abn_mvn_stats': (C.c_int, [_vp, _i64, _i64, C.c_int, _vp, _vp, _vp, _vp]),
    'abn_mvn_apply': (C.c_int, [_vp, _i64, _i64, _vp, _vp, C.c_int, _f32, _vp, _vp]),
    'abn_fbank': (C.c_int, [_vp, C.c_int, _i64, _i32, C.c_double, _i32, _i32,
                             _f32, _vp, _vp, _vp, _i64, _vp, _vp]),
    'abn_fbank_batched': (C.c_int, [_vp, C.c_int, _vp, _vp, _i64, _i32, C.c_double, _i32, _i32,
                                     _f32, _vp, _vp, _vp, _i64, _vp, _vp]),
    'abn_deltas': (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    'abn_deltas_batched': (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    'abn_mfcc': (C.c_int, [_vp, C.c_int, _i64, _i32, C.c_double, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp,
                            _i64, _vp, _i64, _vp]),
    'abn_mfcc_batched': (C.c_int, [_vp, C.c_int, _vp, _vp, _i64, _i32, C.c_double, _i32, _i32, _i32, _f32, _vp, _vp,
                                    _vp, _vp, _i64, _vp, _i64, _vp]),
    'abn_mfcc_path': (C.c_int, [_i32, _i32, _i32]),
    'abn_integrate_ws_bytes': (_i64, [_i64]),
    'abn_integrate_forward': (C.c_int, [_vp, _i64, _vp, _i64, _i64, C.c_int, C.c_int, _f32, _f32, _vp, _vp, _vp, _i64,
                                         C.c_int, _vp, _vp, _vp]),
    'abn_integrate_backward': (C.c_int, [_vp, _i64, _vp, _i64, _i64, C.c_int, C.c_int, _f32, _f32, _vp, _vp, _i64,
                                          C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'abn_knn_ws_bytes': (_i64, [_i64, _i64, C.c_int]),
    'abn_knn_topk': (C.c_int, [_vp, _i64, _vp, _i64, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _i64, _vp]),
    'abn_segment_vectors': (C.c_int, [_vp, _i64, _vp, _vp, _i64, C.c_int, _vp, _vp, _vp]),
    'abn_sample_pairs': (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_int, _vp]),
    'abn_tcl_pairs': (C.c_int, [_vp, _vp, _vp, _i64, _vp, C.c_int, C.c_int, _i64, _i64, C.c_uint64, C.c_uint32, _vp, _vp,
                                _vp, _vp, C.c_int, _i64, _vp]),
    'abn_gmm_max_d': (_i64, []),
    'abn_gmm_max_k': (_i64, []),
    'abn_gmm_posteriors': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    'abn_gmm_ws_bytes': (_i64, [_i64, _i64, _i64, C.c_int]),
    'abn_gmm_accumulate': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, C.c_int, _vp, _i64, _vp]),
    'abn_gmm_mstep': (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, C.c_int, _vp, C.c_double, C.c_double, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _vp, _vp]),
    'abn_kmeans_max_d': (_i64, []),
    'abn_kmeans_max_k': (_i64, []),
    'abn_kmeans_assign': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    'abn_kmeans_ws_bytes': (_i64, [_i64, _i64, _i64, C.c_int]),
    'abn_kmeans_accumulate': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, C.c_int, _vp, _i64, _vp]),
    'abn_kmeans_update': (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'abn_kmeans_viterbi_max_len': (_i64, []),
    'abn_kmeans_viterbi_max_k': (_i64, []),
    'abn_kmeans_viterbi_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'abn_kmeans_viterbi': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _f32, _vp, _vp, _vp, _vp, _i64, _vp]),
    'abn_hmm_max_len': (_i64, []),
    'abn_hmm_max_k': (_i64, []),
    'abn_hmm_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'abn_hmm_forward_backward': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _f32, C.c_int, _vp,
                                           _vp, _vp, _vp, _vp, _i64, _vp]),
    'abn_hmm_forward_backward_stats': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _f32, C.c_int,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'abn_hmm_accumulate_ws_bytes': (_i64, [_i64, _i64, _i64, C.c_int]),
    'abn_hmm_accumulate': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, C.c_int, _vp, _vp, _i64, _vp]),
    'abn_hmm_viterbi_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'abn_hmm_viterbi': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp,
                                  _vp, _i64, _vp]),
    'abn_esk_max_span': (_i64, []),
    'abn_esk_score': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, C.c_int, C.c_int, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    'abn_esk_segment': (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'abn_sd_grid_runs': (_i64, [_i64]),
    'abn_sd_collect': (C.c_int, [_vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'abn_sd_count': (C.c_int, [_vp, _i64, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _i64, _vp, _vp, _vp]),
}
# every symbol include/abnet3_hip_next.h declares (prefix abnx_: entries that are not part of the numbered ABI yet; a later
# change folds them into abnet3_hip.h and SYMBOLS): the twins' arguments plus int32 min_duration at the end
NEXT_SYMBOLS = {
    'abnx_viterbi_dur_max': (_i32, []),
    'abnx_kmeans_viterbi_dur': (C.c_int, SYMBOLS['abn_kmeans_viterbi'][1] + [_i32]),
    'abnx_hmm_viterbi_dur': (C.c_int, SYMBOLS['abn_hmm_viterbi'][1] + [_i32]),
}
# the second section of include/abnet3_hip_next.h (prefix abny_: the HMM with a full transition matrix, csrc/hmm_dense.hip),
# as little part of the numbered ABI as NEXT_SYMBOLS
NEXT2_SYMBOLS = {
    'abny_hmm_dense_max_k': (_i64, []),
    'abny_hmm_dense_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'abny_hmm_dense_forward_backward': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, C.c_int,
                                                  _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
}
# the third section (prefix abnz_: the max-product path of that model, csrc/hmm_dense_vit.hip): abn_hmm_viterbi's arguments
# with li, lt in place of lw, ls, lr
NEXT3_SYMBOLS = {
    'abnz_hmm_dense_viterbi_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'abnz_hmm_dense_viterbi': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp,
                                         _vp, _i64, _vp]),
}
# the fourth section (prefix abnw_: that path with a minimum unit duration): the twin's arguments plus int32 min_duration
# at the end, and a sizing entry of its own
NEXT4_SYMBOLS = {
    'abnw_hmm_dense_viterbi_dur_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'abnw_hmm_dense_viterbi_dur': (C.c_int, NEXT3_SYMBOLS['abnz_hmm_dense_viterbi'][1] + [_i32]),
}
# the fifth section (prefix abnv_: the hard statistics of that model's Viterbi training, csrc/hmm_hard.hip)
NEXT5_SYMBOLS = {
    'abnv_hmm_hard_stats_ws_bytes': (_i64, [_i64, _i64, _i64, _i64, C.c_int]),
    'abnv_hmm_hard_stats': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, C.c_int, _vp, _vp, _vp, _vp, _i64, _vp]),
}
# the sixth section (prefix abnu_: explicit unit durations, csrc/hmm_hsmm.hip): the decoder takes abnz_hmm_dense_viterbi's
# arguments (lx in lt's place) plus ld, ls and int32 L at the end
NEXT6_SYMBOLS = {
    'abnu_hmm_hsmm_max_duration': (_i32, []),
    'abnu_hmm_hsmm_viterbi_ws_bytes': (_i64, [_i64, _i64, _i64, _i64, _i32]),
    'abnu_hmm_hsmm_viterbi': (C.c_int, NEXT3_SYMBOLS['abnz_hmm_dense_viterbi'][1] + [_vp, _vp, _i32]),
    'abnu_hmm_run_stats': (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
}
# the seventh section (prefix abnt_: the in-batch contrastive pair loss, csrc/nce.hip)
NEXT7_SYMBOLS = {
    'abnt_nce_max_d': (_i64, []),
    'abnt_nce_ws_bytes': (_i64, [_i64, _i64]),
    'abnt_nce_loss': (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _i64, _i64, _f32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# the section behind the full term scores (prefix abns_: the pair-free histogram of within-cluster edit distances,
# csrc/edit_hist.hip).  Deliberately NOT a NEXT<n>_SYMBOLS: tests/arg_contract.py enumerates those by name and
# tests/test_arg_contract_host.py demands a row in tests/test_gpu_arg_contract.py for each of their entries; this section is
# held to the same contract by tests/test_gpu_tde_full_contract.py, and folding it into the main ledger is for a change that
# may edit those files
EVAL_SYMBOLS = {
    'abns_edit_hist_max_len': (_i64, []),
    'abns_edit_cluster_hist_ws_bytes': (_i64, [_i64, _i64, _i64]),
    'abns_edit_cluster_hist': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp]),
}
# the section behind the correspondence autoencoder (prefix abnr_: the reconstruction loss and its gradient, csrc/recon.hip).
# A ledger of its own for EVAL_SYMBOLS' reason; tests/test_cae_host.py and tests/test_gpu_cae_contract.py hold it to the contract
CAE_SYMBOLS = {
    'abnr_recon_max_d': (_i64, []),
    'abnr_recon_ws_bytes': (_i64, [_i64, _i64]),
    'abnr_recon_loss': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# the section behind soft-DTW word-pair training (prefix abnq_: the batched soft-DTW forward and backward, csrc/softdtw.hip).
# A ledger of its own for EVAL_SYMBOLS' reason; tests/test_sdtw_host.py and tests/test_gpu_sdtw_contract.py hold it to the contract
SDTW_SYMBOLS = {
    'abnq_softdtw_max_len': (_i64, []),
    'abnq_softdtw_max_d': (_i64, []),
    'abnq_softdtw_ws_bytes': (_i64, [_vp, _vp, _i64, _i64, C.c_int]),
    'abnq_softdtw_forward': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _f32, _vp, _vp, _i64, C.c_int, _vp]),
    'abnq_softdtw_backward': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _f32, _vp, _vp, _vp, _vp, _i64, _vp]),
}
# abn_sd_count's conditions and the limits of abn_sd_collect / abn_sd_count (include/abnet3_hip.h)
SD_CONDITION = {'all': 0, 'swdp': 1, 'swsp': 2}
SD_MAX_N, SD_MAX_THR, SD_MAX_D = 1 << 22, 1 << 30, 4096
# abn_integrate_forward / _backward (include/abnet3_hip.h)
INTEGRATE_MODE = {'sum': 0, 'concat': 1}
W_NONE, W_FIXED, W_SCALAR, W_ATTENTION = range(4)


class TowerDesc(C.Structure):
    """struct abn_tower_desc"""
    _fields_ = [('n_layers', _i32), ('act', _i32), ('last_act', _i32),
                ('batch_norm', _i32), ('dims', _i64 * (MAX_LAYERS + 1))] + [
        (name, _vp * MAX_LAYERS)
        for name in ('W', 'b', 'bn_w', 'bn_b', 'bn_rm', 'bn_rv', 'dW', 'db',
                     'dbn_w', 'dbn_b', 'drop_mask')] + [('precision', _i32), ('d_out_is_dz', _i32), ('defer_reduce', _i32), ('wpack_valid', _i32), ('forward_only', _i32), ('wgrad_part', _i32), ('wpack', _vp), ('drop_seed', _vp), ('drop_p', _f32), ('reserved2_', _i32),
                     ('bn_sync_world', _i32), ('wgrad_split', _i32), ('bn_sync_fn', _vp), ('bn_sync_ctx', _vp), ('n_valid', _vp),
                     ('bn_nbt', _vp * MAX_LAYERS), ('sync_ws', _vp), ('fwd_ws', _vp), ('fwd_calls', _i64), ('source', _vp)]


class StepSource(C.Structure):
    """abn_step_source (include/abnet3_hip.h): a pass's batches as the plan holds them, for steps that need no gather launch."""
    _fields_ = [('table', _vp), ('table_rows', _i64), ('idx1', _vp), ('idx2', _vp), ('labels', _vp), ('steps', _vp), ('step_ctr', _vp)]


class SamplerTables(C.Structure):
    """struct abn_sampler_tables (abn_sample_pairs' tables; abnet3_amd/sampler.py fills it)"""
    POINTERS = ('spk_t', 'type_t', 'type_beg', 'f_t', 'cum_u_t', 'cum_f_t', 'tok_beg', 'toks',
                'spk_s', 'type_s', 's2t', 'spk_beg', 'u_s', 'cum_u_s', 'cum_spk', 'cum_m')
    _fields_ = [('n_cells', _i32), ('n_spk', _i32), ('n_type', _i32), ('n_tok', _i32), ('total', C.c_uint64 * 4)] + [
        (name, _vp) for name in POINTERS]


class OneShotCtx(C.Structure):
    """struct abn_oneshot_ctx (abn_allreduce_oneshot's context)"""
    _fields_ = [('rank', _i32), ('world', _i32), ('mail', _vp * 8), ('cap_floats', _i64)]


class RcclCtx(C.Structure):
    """struct abn_rccl_ctx (abn_rccl_allreduce_f64's context)"""
    _fields_ = [('comm', _vp), ('all_reduce', _vp), ('calls', _i64)]


# abn_allreduce_fn (abn_tower_desc.bn_sync_fn)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class HipLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Returns the bound library; raises HipLibraryError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            'abnet3_amd: %s is missing. Build it with `python -m abnet3_amd.build` '
            '(hipcc, gfx950). There is no CPU fallback.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SYMBOLS.items()) + list(NEXT_SYMBOLS.items()) + list(NEXT2_SYMBOLS.items()) + \
            list(NEXT3_SYMBOLS.items()) + list(NEXT4_SYMBOLS.items()) + list(NEXT5_SYMBOLS.items()) + list(NEXT6_SYMBOLS.items()) + \
            list(NEXT7_SYMBOLS.items()) + list(EVAL_SYMBOLS.items()) + list(CAE_SYMBOLS.items()) + list(SDTW_SYMBOLS.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise HipLibraryError('abnet3_amd: %s does not export %s '
                                  '(stale build?)' % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    if lib.abn_abi_version() != ABI_VERSION:
        raise HipLibraryError('abnet3_amd: ABI version mismatch (library %d, '
                              'binding %d)' % (lib.abn_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def reload_switches():
    """The library reads its A/B switches (ABN_PLANES, ABN_FUSED_MIN_ROWS, ...) from the environment once,
    when it is loaded; tests and A/B tools that change one inside a process call this afterwards."""
    load().abn_reload_switches()


E_ARG = -1
E_WORKSPACE = -3
E_UNSUPPORTED = -4

# abn_tower_path's answers (include/abnet3_hip.h)
PATH_PER_LAYER, PATH_FUSED_F32, PATH_PLANES, PATH_PLANES_INFER, PATH_PLANES_INFER_BN, PATH_BN_LAYERS, PATH_WIDE, PATH_BN_TOWER = range(8)
PRECISION_NAMES = {0: 'fp32', 1: 'bf16', 2: 'bf16x3', 3: 'f16x2'}
# abn_mfcc_path's answers
MFCC_GENERAL, MFCC_WAVE512 = 0, 1
# abn_edit_distance_batched: ABN_EDIT_MAX_SHORT, and the grid cap ABN_EDIT_GRID_BLOCKS x ABN_EDIT_BLOCK_PAIRS = the pairs
# one pass of its grid-stride loop holds
EDIT_MAX_SHORT = 256
EDIT_GRID_BLOCKS, EDIT_BLOCK_PAIRS = 4096, 64
EDIT_GRID_PAIRS = EDIT_GRID_BLOCKS * EDIT_BLOCK_PAIRS

# Which kernels the tower calls of this process took: filled in by model.py from abn_tower_path (a pure
# query with the call's own arguments) while `trace_paths` is on -- tests, bench.py and the trainer's log
# read it.  Python-side bookkeeping: the library itself keeps no record of past calls.
trace_paths = False
last_path = {'forward': -1, 'backward': -1, 'forward_precision': -1, 'backward_precision': -1}


def note_path(desc, x1, x2, rows, n_calls, train, ws, backward):
    if not trace_paths:
        return
    prec = C.c_int32(-1)
    path = load().abn_tower_path(C.byref(desc), ptr(x1), ptr(x2), rows, n_calls, int(train), ptr(ws), int(backward),
                                 C.byref(prec))
    key = 'backward' if backward else 'forward'
    last_path[key] = path
    last_path[key + '_precision'] = prec.value


def last_forward_path():
    return last_path['forward']


def last_backward_path():
    return last_path['backward']


_ON_ERROR = []        # callables run when a library call fails (loss.py: scratch whose "left zero" ticket may be dirty now)


def check(rc, what):
    if rc != 0:
        for hook in _ON_ERROR:
            hook()
        msg = load().abn_last_error()
        raise HipLibraryError('%s failed (%d): %s' % (
            what, rc, msg.decode('utf-8', 'replace') if msg else ''))


def require_device(*tensors):
    """The accelerated path only takes contiguous fp32 HIP tensors."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HipLibraryError(
                'abnet3_amd: expected a tensor on the MI355X (HIP) device, got '
                'device=%s. The accelerated path has no CPU fallback; move the '
                'module and its inputs to the GPU (.cuda()).' % t.device)
        if not t.is_contiguous():
            raise HipLibraryError('abnet3_amd: tensor must be contiguous')


def require_tensor(who, what, t, dtype, rank, width=None):
    """ValueError naming `who` unless `t` is a torch tensor of `dtype` (one dtype, or a tuple of them) with `rank`
    dimensions (and, with `width`, that many columns); then require_device(t).  The check of an argument that reaches a
    kernel as a raw pointer: what require_device alone does not look at."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != rank or \
            (width is not None and t.shape[-1] != width):
        got = '%s %s' % (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
        want = '%d-d %s' % (rank, ' / '.join(str(d).replace('torch.', '') for d in dtypes))
        raise ValueError('%s: %s must be a %s tensor%s, not %s' % (
            who, what, want, '' if width is None else ' of %d columns' % width, got))
    require_device(t)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
