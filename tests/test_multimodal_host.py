"""The multimodal family (abnet3/integration.py, MultimodalSiameseNetwork, MultimodalDataLoader,
MultimodalTrainer) without a GPU: the float64 restatement (mm_np) against the reference's own outputs
(tests/golden/multimodal.npz, tools/make_golden.py G13), construction under seeds, the state_dict / param-group /
description surface, the helpers of utils, and the optimizer's range planning."""
import numpy as np
import pytest
import torch

import mm_np
from conftest import load_golden

CONFIGS = ['concat', 'sum', 'fixed_sum', 'fixed_concat', 'scalar_sum', 'scalar_concat_lr', 'deep_k1_sum',
           'deep_kd_sum', 'deep_k1_concat_async0', 'deep_kd_concat_async1_bn', 'nopost_deep_k1']
UNITS = ['u_sum', 'u_concat', 'u_fixed_sum', 'u_fixed_concat', 'u_scalar_sum', 'u_scalar_concat', 'u_deep_k1_sum',
         'u_deep_kd_sum_tanh', 'u_deep_k1_concat', 'u_deep_kd_concat']


def g13():
    return load_golden('multimodal.npz')


def rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def build(name, seed=None):
    """The port's network of G13 configuration `name` under the generator's seeds (tools/make_golden.py)."""
    from abnet3_amd import integration
    from abnet3_amd.model import MultimodalSiameseNetwork
    cls, ukw, pre, post, nkw = CONFIG_TABLE[name]
    seed = SEEDS[name] if seed is None else seed
    torch.manual_seed(seed)
    np.random.seed(seed)
    unit = getattr(integration, cls)(**ukw)
    return MultimodalSiameseNetwork(integration_unit=unit, pre_integration_net_params=pre,
                                    post_integration_net_params=post, **nkw)


# the G13 configurations, as tools/make_golden.py builds them (its MM_CONFIGS; restated so that the tests do not
# import the generator, which needs the reference checkout)
PRE = [[10, 16, 12], [6, 16, 12]]
CONFIG_TABLE = {
    'concat': ('ConcatenationIntegration', {}, PRE, [24, 8], dict(activation_layer='sigmoid')),
    'sum': ('SumIntegration', {}, PRE, [12, 8], dict(activation_layer='tanh')),
    'fixed_sum': ('BiWeightedFixed', dict(integration_mode='sum', weight_value=0.3), PRE, [12, 8],
                  dict(activation_layer='relu')),
    'fixed_concat': ('BiWeightedFixed', dict(integration_mode='concat'), PRE, [24, 8], dict(activation_layer='sigmoid')),
    'scalar_sum': ('BiWeightedScalarLearnt', dict(integration_mode='sum'), PRE, [12, 8], dict(activation_layer='sigmoid')),
    'scalar_concat_lr': ('BiWeightedScalarLearnt', dict(integration_mode='concat'), PRE, [24, 8],
                         dict(activation_layer='tanh', attention_lr=0.01)),
    'deep_k1_sum': ('BiWeightedDeepLearnt', dict(net_params=[[12, 1], [12, 1]], integration_mode='sum'), PRE, [12, 8],
                    dict(activation_layer='sigmoid')),
    'deep_kd_sum': ('BiWeightedDeepLearnt', dict(net_params=[[12, 12], [12, 12]], integration_mode='sum',
                                                  activation_type='tanh'), PRE, [12, 8], dict(activation_layer='relu')),
    'deep_k1_concat_async0': ('BiWeightedDeepLearnt', dict(net_params=[[10, 4, 1], [6, 4, 1]], integration_mode='concat'),
                              PRE, [24, 8], dict(activation_layer='sigmoid', asynchronous_integration_index=0)),
    'deep_kd_concat_async1_bn': ('BiWeightedDeepLearnt', dict(net_params=[[16, 12], [16, 12]], integration_mode='concat'),
                                 PRE, [24, 8], dict(activation_layer='tanh', asynchronous_integration_index=1,
                                                    batch_norm=True, attention_lr=0.05)),
    'nopost_deep_k1': ('BiWeightedDeepLearnt', dict(net_params=[[12, 1], [12, 1]], integration_mode='sum'), PRE, None,
                       dict(activation_layer='sigmoid')),
}
SEEDS = {name: 1300 + i for i, name in enumerate(CONFIG_TABLE)}


def test_config_table_is_the_fixtures():
    g = g13()
    assert sorted(CONFIG_TABLE) == sorted(CONFIGS)
    for name in CONFIGS:
        assert name + '.arch' in g


@pytest.mark.parametrize('name', UNITS)
def test_mm_np_matches_the_reference_units(name):
    """G13's units alone: output and every gradient of the reference (float32) against the float64 restatement."""
    g = g13()
    mode, kind, x1, x2, gr, w, wc, act_name = mm_np.unit_case(g, name)
    assert rel(mm_np.forward(mode, x1, x2, w, wc), g[name + '.out']) < 1e-6
    dx1, dx2, dz, dw = mm_np.backward(mode, kind, x1, x2, gr, w, wc, act_name)
    assert rel(dx1, g[name + '.dx1']) < 1e-6 and rel(dx2, g[name + '.dx2']) < 1e-6
    if kind == 'attention':
        assert rel(dz, g[name + '.dz']) < 1e-5
    if kind == 'scalar':
        assert rel(dw, g[name + '.dw']) < 1e-5


def test_fixed_weight_is_the_float32_expression():
    """BiWeightedFixed's sum in the reference is fl(fl(w x1) + fl((1 - w) x2)) with w and 1 - w (taken in float64)
    rounded to float32 -- the operands abn_integrate_forward is handed (BiWeightedFixed.kernel_weight)."""
    from abnet3_amd.integration import BiWeightedFixed
    g = g13()
    unit = BiWeightedFixed(integration_mode='sum', weight_value=float(g['u_fixed_sum.w']))
    _, w, wc, _ = unit.kernel_weight()
    x1, x2 = g['u_fixed_sum.x1'], g['u_fixed_sum.x2']
    mine = np.float32(w) * x1 + np.float32(wc) * x2
    assert np.array_equal(mine, g['u_fixed_sum.out'])


@pytest.mark.parametrize('name', CONFIGS)
def test_initial_weights_equal_the_reference(name):
    """Same seeds, same RNG consumption: every tensor, the pre-nets' default initialisation included."""
    g = g13()
    net = build(name)
    sd = net.state_dict()
    ref = {k[len(name + '.init.'):]: v for k, v in g.items() if k.startswith(name + '.init.')}
    assert sorted(sd) == sorted(ref), set(sd) ^ set(ref)
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), ref[k]), k


@pytest.mark.parametrize('name', CONFIGS)
def test_state_dict_keys_are_the_references_plus_the_pre_nets(name):
    net = build(name)
    keys = list(net.state_dict())
    pre = [k for k in keys if k.startswith('pre_nets.')]
    rest = [k for k in keys if not k.startswith('pre_nets.')]
    assert all(k.startswith('integration_unit.') or k.startswith('post_net.') for k in rest), rest
    assert len(pre) == sum(len(list(pn.state_dict())) for pn in net.pre_nets)
    assert pre[0].startswith('pre_nets.0.0.')


@pytest.mark.parametrize('name', CONFIGS)
def test_parameters_are_param_groups(name):
    net = build(name)
    groups = net.parameters()
    assert all(isinstance(gr, dict) for gr in groups)
    unit = list(net.integration_unit.parameters())
    every = sum((list(pn.parameters()) for pn in net.pre_nets), []) + \
        (list(net.post_net.parameters()) if net.post else []) + unit
    lr = net.attention_lr
    if lr:
        assert len(groups) == 2 and groups[1]['lr'] == lr and 'lr' not in groups[0]
        assert [id(p) for p in groups[1]['params']] == [id(p) for p in unit]
    else:
        assert len(groups) == 1
    assert sorted(id(p) for gr in groups for p in gr['params']) == sorted(id(p) for p in every)


@pytest.mark.parametrize('name', CONFIGS)
def test_architecture_str_and_whoami(name):
    g = g13()
    net = build(name)
    assert net.architecture_str() == str(g[name + '.arch'])
    who = net.whoami()
    assert who['class_name'] == 'MultimodalSiameseNetwork'
    assert who['architecture'] == str(g[name + '.arch'])
    assert '_flat' not in who['params']


def test_freeze_training_is_the_references_set():
    """The post-net and the unit (the reference's registered modules); start_training gives the unit back."""
    net = build('deep_k1_sum')
    net.freeze_training()
    assert not any(p.requires_grad for p in net.post_net.parameters())
    assert not any(p.requires_grad for p in net.integration_unit.parameters())
    assert all(p.requires_grad for pn in net.pre_nets for p in pn.parameters())
    net.integration_unit.start_training()
    assert all(p.requires_grad for p in net.integration_unit.parameters())


def test_units_surface():
    from abnet3_amd import integration
    np.random.seed(5)
    u = integration.BiWeightedFixed(weight_value=0)          # 0 is redrawn, as None is
    np.random.seed(5)
    assert u.weight == np.random.random()
    with pytest.raises(AssertionError):
        integration.BiWeightedFixed(weight_value=1.5)
    with pytest.raises(AssertionError):
        integration.BiWeightedFixed(integration_mode='mean')
    s = integration.BiWeightedScalarLearnt(weight_value=0.25)
    assert list(s.state_dict()) == ['weight'] and s.weight.requires_grad
    s.set_headstart_weight(0.5)
    assert float(s.weight) == 0.5 and not s.weight.requires_grad
    d = integration.BiWeightedDeepLearnt(net_params=[[7, (5, 2), 3], [4, 3]], activation_type='tanh')
    assert d.K == 3 and len(d.linear1) == 5 and isinstance(d.linear1[1], torch.nn.Tanh)
    assert sorted(d.state_dict()) == ['linear1.0.bias', 'linear1.0.weight', 'linear1.2.bias', 'linear1.2.weight',
                                      'linear1.4.bias', 'linear1.4.weight', 'linear2.0.bias', 'linear2.0.weight']
    d.set_headstart_weight(0.3)
    assert d.freezed and float(d.get_weights()) == pytest.approx(0.3)
    kind, w, wc, _ = d.kernel_weight()
    assert w == float(np.float32(0.3)) and wc == float(np.float32(1) - np.float32(0.3))
    assert str(integration.SumIntegration()) == 'SumIntegration\nIntegration method: sum\n'


def test_expand_dimension_list_and_to_ordinal():
    from abnet3_amd.utils import expand_dimension_list, to_ordinal
    assert expand_dimension_list([280, (500, 2), [7, 3], 100]) == [280, 500, 500, 7, 7, 7, 100]
    with pytest.raises(TypeError):
        expand_dimension_list([1.5])
    assert [to_ordinal(n) for n in (1, 2, 3, 4, 11, 12, 13, 21, 22, 23, 101, 111)] == \
        ['1st', '2nd', '3rd', '4th', '11th', '12th', '13th', '21st', '22nd', '23rd', '101st', '111st']


def _optimizer(net, lr=0.1):
    from abnet3_amd.trainer import FlatOptimizer
    net.flatten_parameters()
    for p in net.live_parameters():
        p.grad = torch.zeros_like(p)
    return FlatOptimizer(net, 'adam', lr)


def test_range_planning_one_range_without_attention_lr():
    net = build('deep_k1_sum')
    opt = _optimizer(net)
    (first, n, lr, step, members), = opt.ranges()
    live = net.live_parameters()
    assert first == 0 and n == net._offsets[-1] + live[-1].numel() and lr == 0.1 and step == 1
    assert members == list(range(len(live)))


def test_range_planning_attention_lr_and_frozen_ranges():
    net = build('deep_kd_concat_async1_bn')
    opt = _optimizer(net)
    rs = opt.ranges()
    assert [(r[2], r[3]) for r in rs] == [(0.1, 1), (0.05, 1)]
    unit = {id(p) for p in net.integration_unit.parameters()}
    live = net.live_parameters()
    assert all(id(live[i]) in unit for i in rs[1][4]) and not any(id(live[i]) in unit for i in rs[0][4])
    # headstart (k, False, w): the post-net stops, the pre-nets and the attention go on
    net.freeze_training()
    net.integration_unit.start_training()
    for p in net.post_net.parameters():
        p.grad = None
    rs = opt.ranges()
    post = {id(p) for p in net.post_net.parameters()}
    covered = [i for r in rs for i in r[4]]
    assert not any(id(live[i]) in post for i in covered)
    assert len(covered) == len(live) - len(post)
    for first, n, _, _, members in rs:       # a range is one contiguous run of the flat buffer
        assert first == net._offsets[members[0]] and first + n == net._offsets[members[-1]] + live[members[-1]].numel()


def test_range_planning_keeps_step_counts_per_parameter():
    """A parameter that joins later starts at step 1 (Adam's bias correction, SGD's first momentum step)."""
    net = build('deep_k1_sum')
    opt = _optimizer(net)
    live = net.live_parameters()
    unit = {id(p) for p in net.integration_unit.parameters()}
    opt.ranges()
    opt._steps = [0 if id(p) in unit else 1 for p in live]        # the unit sat out the first step
    rs = opt.ranges()
    assert len(rs) == 2
    for first, n, lr, step, members in rs:
        assert step == (1 if id(live[members[0]]) in unit else 2)
        assert len({id(live[i]) in unit for i in members}) == 1


def test_siamese_network_keeps_one_launch():
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import FlatOptimizer
    net = SiameseNetwork(input_dim=4, num_hidden_layers=1, hidden_dim=6, output_dim=3, activation_layer='sigmoid')
    assert FlatOptimizer(net, 'sgd', 0.1).ranges() is None


def test_loader_consistency_check():
    from abnet3_amd.dataloader import MultimodalDataLoader
    dl = MultimodalDataLoader('unused', ['a', 'b'])
    assert dl.batch_size == 500 and dl.randomize_dataset is False
    a = {'u0': np.zeros((5, 3)), 'u1': np.zeros((4, 3))}
    dl.check_consistency([a, {'u0': np.zeros((5, 2)), 'u1': np.zeros((4, 2))}])
    with pytest.raises(ValueError):
        dl.check_consistency([a, {'u0': np.zeros((5, 2))}])
    with pytest.raises(ValueError):
        dl.check_consistency([a, {'u0': np.zeros((5, 2)), 'u1': np.zeros((3, 2))}])
