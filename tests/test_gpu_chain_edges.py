"""Edges of the operand-plane chains (csrc/tower_planes.h) that the k-loop's peeled tail and the data-gradient
chain's loss phase reach: layers of exactly PL_DEPTH steps (the k-loop is its tail alone), K-split halves of
PL_DEPTH steps, an odd block count on two-block waves with a 4-wide embedding (most loss-phase lanes idle), C2's
widths, an embedding wider than one loss-phase pass -- at 256 rows (the fewest the plane launches take by
themselves) and at 272 (one workgroup holds rows of both towers, the last one 16 rows).  direct_forward +
direct_backward_loss against oracle/torch_ref in float64, with the tolerances tests/test_gpu_planes.py uses for the
same quantities.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest
import torch

from conftest import rel_err, check_grads

pytestmark = pytest.mark.gpu

TOL, GTOL = 1e-5, 1e-4          # tests/test_gpu_planes.py: embeddings (loss: 10 x), gradients -- bf16x3 and f16x2 alike

TOWERS = [  # (input, hidden, hidden layers, output)
    (40, 64, 2, 100),       # every layer is exactly PL_DEPTH steps: tail only
    (40, 128, 2, 100),      # the K-split path, whose halves are PL_DEPTH steps each
    (40, 288, 1, 4),        # nine output blocks (two-block waves, odd count); a 4-wide embedding
    (40, 500, 2, 100),      # C2's shapes
    (40, 64, 1, 256),       # output / 4 > 32: the loss phase's loop runs twice per lane
]
PAIRS = [128, 136]
LOSSES = [('coscos2', False), ('coscos2', True), ('cosmargin', True), ('cosmargin', False)]
MARGIN = 0.3


@pytest.fixture(autouse=True)
def planes_forced(monkeypatch):
    monkeypatch.setenv('ABN_FUSED_MIN_ROWS', '0')
    monkeypatch.setenv('ABN_PLANES', '1')
    monkeypatch.setenv('ABN_WIDE', '0')


def tower_kw(tower):
    d_in, hid, nh, d_out = tower
    return dict(input_dim=d_in, num_hidden_layers=nh, hidden_dim=hid, output_dim=d_out, activation_layer='sigmoid',
                p_dropout=0.0, batch_norm=False)


def build(tower, precision):
    from abnet3_amd.model import SiameseNetwork
    torch.manual_seed(tower[1] + tower[3])
    net = SiameseNetwork(**tower_kw(tower)).cuda()
    net.precision = precision
    net.train()
    return net


def batch(tower, B, seed=0, labels=(1, -1)):
    rng = np.random.default_rng(1000 * seed + B + tower[1])
    x1 = rng.standard_normal((B, tower[0])).astype(np.float32)
    x2 = rng.standard_normal((B, tower[0])).astype(np.float32)
    return x1, x2, rng.choice(labels, B)


_ORACLE = {}


def oracle(tower, B, n_valid=None):
    """float64 embeddings of the B pairs, and per loss (value, gradients) over the first n_valid of them (all: None):
    computed once per case, shared and left alone."""
    key = (tower, B, n_valid)
    if key not in _ORACLE:
        from oracle import torch_ref
        ref = torch_ref.RefSiamese(**tower_kw(tower)).double()
        ref.load_state_dict({k: v.detach().cpu().double() for k, v in build(tower, 'bf16x3').state_dict().items()})
        ref.train()
        x1, x2, y = batch(tower, B)
        e1, e2 = ref(torch.from_numpy(x1).double(), torch.from_numpy(x2).double())
        n = B if n_valid is None else n_valid
        res = {}
        for lname, avg in LOSSES:
            ref.zero_grad()
            lv = torch_ref.pair_loss(e1[:n], e2[:n], torch.from_numpy(y[:n]), lname, MARGIN, avg)
            lv.backward(retain_graph=True)
            res[lname, avg] = (float(lv.detach()), {k: q.grad.numpy().copy() for k, q in ref.named_parameters()})
        _ORACLE[key] = (torch.cat([e1, e2]).detach().numpy(), res)
    return _ORACLE[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(net, x1, x2, y, lname, avg, **kw):
    from abnet3_amd import _lib
    for q in net.parameters():
        q.grad = None
    emb, state = net.direct_forward(x1, x2)
    lv = net.direct_backward_loss(state, y, lname, MARGIN, avg, **kw)
    assert lv is not None
    assert _lib.last_forward_path() == _lib.PATH_PLANES and _lib.last_backward_path() == _lib.PATH_PLANES
    return emb, lv


def grads_of(net):
    return {k: q.grad.cpu().numpy() for k, q in net.named_parameters()}


def check(net, emb, lv, ref_emb, ref_loss, ref_grads, tag):
    if ref_emb is not None:
        e = rel_err(emb.cpu().numpy(), ref_emb)
        print(tag, 'embeddings', e)
        assert e < TOL, tag
    d = abs(float(lv) - ref_loss)
    print(tag, 'loss', float(lv), ref_loss, d)
    assert d <= 10 * TOL * abs(ref_loss) + 1e-6, tag
    check_grads(grads_of(net), ref_grads, list(ref_grads), False, tol=GTOL)


@pytest.mark.parametrize('B', PAIRS)
@pytest.mark.parametrize('tower', TOWERS)
def test_embeddings_loss_and_gradients_against_the_oracle(tower, B, split):
    ref_emb, ref = oracle(tower, B)
    net = build(tower, split)
    x1, x2, y = (dev(a) for a in batch(tower, B))
    for lname, avg in LOSSES:
        emb, lv = run(net, x1, x2, y, lname, avg)
        check(net, emb, lv, ref_emb, *ref[lname, avg], tag=(tower, B, split, lname, avg))


@pytest.mark.parametrize('tower', TOWERS)
def test_every_label_type_gives_the_same_bits(tower, split):
    """int8, int32, int64, float32, float64 labels (1, -1 and 0 among them): one loss, one set of gradients."""
    B = 136
    net = build(tower, split)
    x1, x2, y = batch(tower, B, seed=1, labels=(1, -1, 0))
    x1, x2 = dev(x1), dev(x2)
    for lname, avg in (('coscos2', False), ('cosmargin', True)):
        first = None
        for dt in (torch.int64, torch.int8, torch.int32, torch.float32, torch.float64):
            emb, lv = run(net, x1, x2, dev(y).to(dt), lname, avg)
            got = (lv.clone(), [q.grad.clone() for q in net.parameters()])
            if first is None:
                first = got
                continue
            assert torch.equal(got[0], first[0]), (dt, float(got[0]), float(first[0]))
            for (k, _), a, b in zip(net.named_parameters(), got[1], first[1]):
                assert torch.equal(a, b), (dt, k)


@pytest.mark.parametrize('tower', [TOWERS[0], TOWERS[2], TOWERS[3]])
def test_real_pair_count_on_a_padded_batch(tower, split):
    """n_valid < B: the pairs behind it (here: ordinary rows, not zeros) give no loss term and no gradient, and
    avg divides by n_valid -- the oracle on the first n_valid pairs alone."""
    B, nv = 136, 101
    ref_emb, ref = oracle(tower, B, nv)
    net = build(tower, split)
    x1, x2, y = (dev(a) for a in batch(tower, B))
    n_valid = torch.tensor([nv], dtype=torch.int32, device='cuda')
    for lname, avg in LOSSES:
        emb, lv = run(net, x1, x2, y, lname, avg, n_valid=n_valid)
        check(net, emb, lv, ref_emb, *ref[lname, avg], tag=(tower, B, nv, split, lname, avg))


@pytest.mark.parametrize('tower,B', [(TOWERS[3], 136), (TOWERS[0], 128), (TOWERS[2], 136)])
def test_three_launches_back_to_back_keep_their_losses_apart(tower, B, split):
    """Three backward-with-loss launches on different batches with no synchronisation between them: each loss is
    the one its batch gives alone, loss_accum their sum, and the ticket counter reads zero afterwards."""
    from abnet3_amd import _lib
    net = build(tower, split)
    batches = [tuple(dev(a) for a in batch(tower, B, seed=s)) for s in range(3)]
    alone = []
    for x1, x2, y in batches:
        emb, lv = run(net, x1, x2, y, 'coscos2', False)
        alone.append(float(lv))
        torch.cuda.synchronize()
    assert len(set(alone)) == 3
    need = _lib.load().abn_tower_backward_loss_ws_bytes(2 * B)
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    accum = torch.zeros((), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    got = [run(net, x1, x2, y, 'coscos2', False, loss_ws=ws, loss_accum=accum)[1] for x1, x2, y in batches]
    torch.cuda.synchronize()
    assert [float(v) for v in got] == alone
    assert float(accum) == (alone[0] + alone[1]) + alone[2]          # (float32 losses: their float64 sum is exact)
    assert int(ws[:4].view(torch.int32)) == 0
