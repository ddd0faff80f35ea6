"""What the per-utterance entries (kmeans.viterbi, hmm.forward_backward, hmm.viterbi and their full-transition twins)
share on the host: the checks of the table, of the utterances' offsets and lengths, of a minimum duration and of a
caller's output tensors, the result tensors, and the workspace with the offsets and lengths uploaded beside it."""
import numpy as np
import torch

from . import _lib


def starts(lens):
    """First rows [n] int64 of utterances of the given lengths laid end to end."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.cumsum(lens) - lens


def table_shape(who, table):
    """(T, D) of a [T, D] float32 tensor, or ValueError: the first host check of every entry of hmm.py."""
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype != torch.float32:      # (host checks first)
        raise ValueError('%s: a [T, D] float32 table is needed' % who)
    return table.shape


def check_ids(who, ids, T):
    """ValueError unless a caller's `ids` (None: the entry makes its own) is a contiguous [T] int32 tensor."""
    if ids is not None and (not isinstance(ids, torch.Tensor) or ids.shape != (T,) or ids.dtype != torch.int32 or
                            not ids.is_contiguous()):
        raise ValueError('%s: ids must be a contiguous [T] int32 tensor' % who)


def path_results(ids, T, n_utt, want_log_prob, device):
    """(ids, log_prob or None, n_switch or None, n_good) on the device, what a max-product entry fills: a fresh `ids` holds
    -1, the per-utterance results 0."""
    if ids is None:
        ids = torch.full((T,), -1, dtype=torch.int32, device=device)
    _lib.require_device(ids)
    lp = torch.zeros(n_utt, dtype=torch.float64, device=device) if want_log_prob else None
    nsw = torch.zeros(n_utt, dtype=torch.int32, device=device) if want_log_prob else None
    return ids, lp, nsw, torch.zeros(n_utt, dtype=torch.int32, device=device)


def posterior_table(who, out, T, K, device):
    """A caller's `out`, checked, or a fresh table of zeros: the contiguous [T, K] float32 device tensor a forward-backward
    entry writes."""
    if out is None:
        out = torch.zeros((T, K), dtype=torch.float32, device=device)
    if out.shape != (T, K) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError('%s: out must be a contiguous [T, K] float32 tensor' % who)
    _lib.require_device(out)
    return out


def utterance_spans(who, off, lens, T, longest_allowed, limit_name):
    """(off int64 [n_utt], lens int64 [n_utt], n_utt, longest) as host arrays, or ValueError: as many offsets as lengths,
    every utterance inside the table's T rows, no two overlapping, none longer than longest_allowed (the value of the
    library's limit_name).  off, lens: host sequences or device tensors."""
    host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    off_h, len_h = host(off).astype(np.int64).ravel(), host(lens).astype(np.int64).ravel()
    n_utt = len(off_h)
    if len(len_h) != n_utt:
        raise ValueError('%s: %d offsets and %d lengths' % (who, n_utt, len(len_h)))
    if n_utt and ((off_h < 0).any() or (len_h < 0).any() or (off_h + len_h > T).any()):
        raise ValueError('%s: an utterance lies outside the table\'s %d rows' % (who, T))
    if n_utt > 1:
        order = np.argsort(off_h, kind='stable')
        if (off_h[order][1:] < (off_h + len_h)[order][:-1]).any():
            raise ValueError('%s: utterances overlap' % who)
    longest = int(len_h.max()) if n_utt else 0
    if longest > longest_allowed:
        raise ValueError('%s: an utterance of %d frames, the kernel takes up to %d (%s)' % (who, longest, longest_allowed, limit_name))
    return off_h, len_h, n_utt, longest


def viterbi_dur_max():
    """The largest minimum duration the max-product kernels take (abnx_viterbi_dur_max)."""
    return int(_lib.load().abnx_viterbi_dur_max())


def check_min_duration(who, min_duration):
    """min_duration as an int, or ValueError: an integer 1 .. viterbi_dur_max()."""
    if isinstance(min_duration, bool) or not isinstance(min_duration, (int, np.integer)) or \
            not 1 <= int(min_duration) <= viterbi_dur_max():
        raise ValueError('%s: min_duration = %r, an integer 1 .. %d is needed (abnx_viterbi_dur_max)'
                         % (who, min_duration, viterbi_dur_max()))
    return int(min_duration)


def workspace(who, ws_bytes_fn, off_h, len_h, longest, K, D, device):
    """(ws uint8, off int64, lens int32) on the device: the workspace ws_bytes_fn (a *_ws_bytes entry of the library) asks
    for, its refusal as a ValueError, and the utterances uploaded."""
    need = ws_bytes_fn(len(off_h), longest, K, D)
    if need < 0:
        raise ValueError('%s: %s' % (who, _lib.load().abn_last_error().decode('utf-8', 'replace')))
    ws = torch.empty(int(need), dtype=torch.uint8, device=device)
    return ws, torch.from_numpy(off_h).to(device), torch.from_numpy(len_h.astype(np.int32)).to(device)
