"""Integration units on MI355X: the class surface of abnet3/integration.py.

Mirrors (file:line relative to the reference checkout)
  IntegrationUnitBuilder    abnet3/integration.py:23-67
  ConcatenationIntegration  abnet3/integration.py:71-92
  SumIntegration            abnet3/integration.py:94-117
  BiWeightedFixed           abnet3/integration.py:252-307
  BiWeightedScalarLearnt    abnet3/integration.py:310-342
  BiWeightedDeepLearnt      abnet3/integration.py:345-475
Same constructor kwargs, asserts, RNG consumption, state_dict keys, save / load, __str__, set_headstart_weight and
start_training.  The units are parameter holders and describe their weight; the arithmetic -- the weighted sum or
concatenation and its backward -- is ONE launch per direction (abn_integrate_forward / abn_integrate_backward,
csrc/integrate.hip), and BiWeightedDeepLearnt's two attention nets run as tower segments of the
MultimodalSiameseNetwork that owns the unit.  MultitaskIntegration and BiWeightedPreTrained are not ported.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .utils import expand_dimension_list

activation_functions = {'relu': nn.ReLU,
                        'sigmoid': nn.Sigmoid,
                        'tanh': nn.Tanh}

init_functions = {'xavier_uni': nn.init.xavier_uniform_,
                  'xavier_normal': nn.init.xavier_normal_,
                  'orthogonal': nn.init.orthogonal_}


class IntegrationUnitBuilder(nn.Module):
    """Base class for integration units (abnet3/integration.py:23-67)."""

    def __init__(self, output_path="", cuda_bool=False, *args, **kwargs):
        super(IntegrationUnitBuilder, self).__init__()
        self.output_path = output_path
        self.cuda_bool = cuda_bool

    def integration_method(self, *args, **kwargs):
        raise NotImplementedError('Unimplemented integration_method for class:',
                                  self.__class__.__name__)

    def forward(self, *args, **kwargs):
        raise NotImplementedError('Unimplemented forward for class:',
                                  self.__class__.__name__)

    def whoami(self, *args, **kwargs):
        raise NotImplementedError('Unimplemented whoami for class:',
                                  self.__class__.__name__)

    def save(self, epoch=''):
        torch.save(self.state_dict(), self.output_path + epoch + 'integration.pth')

    def load(self, path=None):
        self.load_state_dict(torch.load(path + 'integration.pth', map_location='cpu'))

    def __str__(self):
        return str(self.__class__.__name__)

    # -- what abn_integrate_forward needs -------------------------------------------------------------------------
    mode = 'sum'

    def kernel_weight(self):
        """(weight kind, w, 1 - w, learnt scalar parameter | None) of the next forward (_lib.W_*)."""
        return _lib.W_NONE, 1.0, 1.0, None


class ConcatenationIntegration(IntegrationUnitBuilder):

    mode = 'concat'

    def __init__(self, *args, **kwargs):
        super(ConcatenationIntegration, self).__init__(*args, **kwargs)

    def forward(self, x_list, *args, **kwargs):
        return integrate_list(self, x_list)

    def __str__(self):
        _str = str(self.__class__.__name__)
        _str += "\nIntegration method: concatenation\n"
        return _str


class SumIntegration(IntegrationUnitBuilder):

    mode = 'sum'

    def __init__(self, *args, **kwargs):
        super(SumIntegration, self).__init__(*args, **kwargs)

    def forward(self, x_list, *args, **kwargs):
        return integrate_list(self, x_list)

    def __str__(self):
        _str = str(self.__class__.__name__)
        _str += "\nIntegration method: sum\n"
        return _str


class BiWeightedFixed(IntegrationUnitBuilder):
    """w * x1 (+ | concatenated with) (1 - w) * x2, w fixed (abnet3/integration.py:252-307).  As in the
    reference a weight_value of None OR 0 draws np.random.random()."""

    def __init__(self, integration_mode="sum", weight_value=None, *args, **kwargs):
        super(BiWeightedFixed, self).__init__(*args, **kwargs)
        assert integration_mode in ("sum", "concat"), "Only sum and concat supported"
        if not weight_value:
            weight_value = np.random.random()
        else:
            assert weight_value >= 0, "weight must be greater or equal to 0"
            assert weight_value <= 1, "weight must be less or equal to 1"
        self.weight = weight_value
        self.weight_complement = 1 - self.weight
        self.integration_mode = integration_mode

    @property
    def mode(self):
        return self.integration_mode

    def get_weights(self):
        return self.weight

    def kernel_weight(self):
        # torch.mul(x, python float): the float is rounded to float32 first, and so is 1 - w (taken in float64)
        return _lib.W_FIXED, float(np.float32(self.weight)), float(np.float32(self.weight_complement)), None

    def forward(self, x_list, *args, **kwargs):
        assert len(x_list) == 2, "BiWeighted integrators use two modalities"
        return integrate_list(self, x_list)

    def __str__(self):
        _str = ""
        _str += str(self.__class__.__name__)
        _str += "\n"
        _str += "Integration method: {}\n".format(self.integration_mode)
        _str += "Weight value: {}\n".format(self.weight)
        return _str


class BiWeightedScalarLearnt(BiWeightedFixed):
    """The weight is one learnt scalar (abnet3/integration.py:310-342); 1 - w is taken in float32."""

    def __init__(self, *args, **kwargs):
        super(BiWeightedScalarLearnt, self).__init__(*args, **kwargs)
        self.weight = nn.Parameter(torch.Tensor([self.weight]))
        self.start_training()

    @property
    def weight_complement(self):
        return torch.add(torch.mul(self.weight.detach(), -1), 1)

    @weight_complement.setter
    def weight_complement(self, value):
        pass                    # (derived from the weight at every forward, as the reference recomputes it)

    def set_headstart_weight(self, headstart_weight):
        self.weight.data[0] = headstart_weight
        self.weight.requires_grad = False

    def start_training(self):
        self.weight.requires_grad = True

    def kernel_weight(self):
        return _lib.W_SCALAR, 0.0, 0.0, self.weight

    def __str__(self):
        _str = ""
        _str += str(self.__class__.__name__)
        _str += "\n"
        _str += "Integration method: {}\n".format(self.integration_mode)
        _str += "Actual weight value: {}\n".format(self.weight)
        return _str


class BiWeightedDeepLearnt(BiWeightedFixed):
    """w = act(linear1(d1) + linear2(d2)) per row (K = 1) or per feature (K = width), K being the last entry of
    net_params[0] (abnet3/integration.py:345-475).  linear1 / linear2 are nn.Sequential parameter holders; the
    MultimodalSiameseNetwork that owns the unit runs them as tower segments (activation_type between the layers,
    none after the last) and the activation of their sum inside abn_integrate_forward.  get_weights() is the w of
    the last forward_once call (during a headstart: the fixed scalar, the attention nets are not evaluated)."""

    def __init__(self, net_params, activation_type="sigmoid",
                 init_type='xavier_uni', *args, **kwargs):
        super(BiWeightedDeepLearnt, self).__init__(*args, **kwargs)
        assert activation_type in ('sigmoid', 'tanh')
        assert init_type in ('xavier_uni', 'xavier_normal', 'orthogonal')

        self.input_dim1 = net_params[0][0]
        self.input_dim2 = net_params[1][0]
        self.activation_layer = activation_functions[activation_type]()
        self.activation_type = activation_type
        self.init_function = init_functions[init_type]
        self.freezed = False

        self.weight = torch.rand(1)
        self.weight_complement = torch.add(torch.mul(self.weight, -1), 1)

        self.linear1 = self.build_net(net_params[0], self.activation_type)
        self.linear2 = self.build_net(net_params[1], self.activation_type)
        assert self.linear1[-1].out_features == self.linear2[-1].out_features, \
            'both attention nets must end at the same width'
        self.apply(self.init_weight_method)
        self.start_training()
        self._last_w = None

    @property
    def K(self):
        return self.linear1[-1].out_features

    def build_net(self, dimensions_list, activation_type):
        dimensions_list = expand_dimension_list(dimensions_list)
        layers = []
        for idx in range(len(dimensions_list) - 1):
            in_dim = dimensions_list[idx]
            out_dim = dimensions_list[idx + 1]
            layers.append(nn.Linear(in_dim, out_dim))
            if idx != len(dimensions_list) - 2:
                layers.append(activation_functions[activation_type]())
        return nn.Sequential(*layers)

    def init_weight_method(self, layer):
        if isinstance(layer, nn.Linear):
            self.init_function(layer.weight.data,
                               gain=nn.init.calculate_gain(self.activation_type))
            layer.bias.data.fill_(0.0)

    def set_headstart_weight(self, headstart_weight):
        self.weight = torch.Tensor([headstart_weight])
        self.weight_complement = torch.add(torch.mul(self.weight, -1), 1)
        self.freezed = True
        for param in self.parameters():
            param.requires_grad = False

    def start_training(self):
        self.freezed = False
        for param in self.parameters():
            param.requires_grad = True

    def get_weights(self):
        if self.freezed or self._last_w is None:
            return self.weight
        return self._last_w

    def kernel_weight(self):
        if self.freezed:         # torch.Tensor([w]): float32, and 1 - w in float32
            w = np.float32(self.weight[0].item())
            return _lib.W_FIXED, float(w), float(np.float32(1.0) - w), None
        return _lib.W_ATTENTION, 0.0, 0.0, None

    def forward(self, x_list, diff_input=None, *args, **kwargs):
        raise NotImplementedError('abnet3_amd: BiWeightedDeepLearnt runs inside a MultimodalSiameseNetwork (its '
                                  'attention nets are tower segments of that network)')

    def __str__(self):
        _str = ""
        _str += str(self.__class__.__name__)
        _str += "\n"
        _str += "Integration method: {}\n".format(self.integration_mode)
        if self.input_dim2:
            _str += "Input dims:    ({}, {})\n".format(self.input_dim1,
                                                       self.input_dim2)
        else:
            _str += "Input dims:    ({0}, {0})\n".format(self.input_dim1)
        _str += "Activation:    {}\n".format(self.activation_type)
        _str += "\nLinear 1:\n{}".format(str(self.linear1))
        _str += "\nLinear 2:\n{}".format(str(self.linear2))
        _str += "\nAct Layer:     {}\n".format(str(self.activation_type))
        return _str


# -- the launches ----------------------------------------------------------------------------------------------

class _IntegrateFunction(torch.autograd.Function):
    """abn_integrate_forward and its backward.  `spec` = (mode, kind, w, 1 - w, K, act, grad slot | None, holder):
    the learnt scalar's gradient lands in `grad slot(...)` (its view of the network's flat gradient buffer) when
    one is given; holder.w receives the forward's w."""

    @staticmethod
    def forward(ctx, spec, x1, x2, z1, z2, wparam):
        mode, kind, wf, wc, K, act, slot, holder = spec
        lib = _lib.load()
        for t in (x1, x2, z1, z2):
            if t is not None and (t.dim() != 2 or t.dtype != torch.float32):
                raise ValueError('abnet3_amd: an integration unit takes [rows, d] float32 inputs, not %s %s' % (tuple(t.shape), t.dtype))
        x1, x2 = x1.contiguous(), x2.contiguous()
        z1 = z1.contiguous() if z1 is not None else None
        z2 = z2.contiguous() if z2 is not None else None
        _lib.require_device(x1, x2, z1, z2, wparam)
        rows, d1, d2 = x1.shape[0], x1.shape[1], x2.shape[1]
        if x2.shape[0] != rows:
            raise ValueError('abnet3_amd: the two modalities must have the same number of rows')
        if mode == 'sum' and d2 != d1:
            raise ValueError('abnet3_amd: a sum of two modalities needs inputs of one width, not %d and %d' % (d1, d2))
        if any(z is not None and tuple(z.shape) != (rows, K) for z in (z1, z2)):
            raise ValueError('abnet3_amd: the attention nets\' outputs must be [%d, %d]' % (rows, K))
        dout = d1 if mode == 'sum' else d1 + d2
        out = torch.empty(rows, dout, dtype=torch.float32, device=x1.device)
        w_out = torch.empty(rows, K, dtype=torch.float32, device=x1.device) if kind == _lib.W_ATTENTION else None
        _lib.check(lib.abn_integrate_forward(
            _lib.ptr(x1), d1, _lib.ptr(x2), d2, rows, _lib.INTEGRATE_MODE[mode], kind, wf, wc, _lib.ptr(wparam),
            _lib.ptr(z1), _lib.ptr(z2), K, act, _lib.ptr(out), _lib.ptr(w_out), _lib.stream()), 'abn_integrate_forward')
        if holder is not None:
            holder.w = w_out
        ctx.spec = spec
        ctx.save_for_backward(x1, x2, w_out, wparam)
        return out

    @staticmethod
    def backward(ctx, g):
        mode, kind, wf, wc, K, act, slot, holder = ctx.spec
        x1, x2, w, wparam = ctx.saved_tensors
        lib = _lib.load()
        g = g.contiguous()
        _lib.require_device(g)
        rows = x1.shape[0]
        need = ctx.needs_input_grad
        dx1 = torch.empty_like(x1) if need[1] else None
        dx2 = torch.empty_like(x2) if need[2] else None
        dz = torch.empty(rows, K, dtype=torch.float32, device=g.device) if kind == _lib.W_ATTENTION and (need[3] or need[4]) else None
        dw, ws = None, None
        if kind == _lib.W_SCALAR and need[5]:
            dw = slot() if slot is not None else torch.empty(1, dtype=torch.float32, device=g.device)
            from .loss import _scratch
            ws = _scratch(lib.abn_integrate_ws_bytes(rows), g.device)
        _lib.check(lib.abn_integrate_backward(
            _lib.ptr(x1), x1.shape[1], _lib.ptr(x2), x2.shape[1], rows, _lib.INTEGRATE_MODE[mode], kind, wf, wc,
            _lib.ptr(wparam), _lib.ptr(w), K, act, _lib.ptr(g), _lib.ptr(dx1), _lib.ptr(dx2), _lib.ptr(dz), _lib.ptr(dw),
            _lib.ptr(ws), _lib.stream()), 'abn_integrate_backward')
        return None, dx1, dx2, dz if need[3] else None, dz if need[4] else None, dw


def integrate(unit, x1, x2, z1=None, z2=None, slot=None, holder=None):
    """The unit's integration of two [rows, d] inputs (z1 / z2: the attention nets' outputs, BiWeightedDeepLearnt)."""
    kind, wf, wc, wparam = unit.kernel_weight()
    K, act = 1, _lib.ACT['sigmoid']
    if kind == _lib.W_ATTENTION:
        K, act = unit.K, _lib.ACT[unit.activation_type]
    if x1.shape[0] == 0 and kind != _lib.W_SCALAR:
        _lib.require_device(x1, x2)
        return x1.new_zeros((0, x1.shape[1] if unit.mode == 'sum' else x1.shape[1] + x2.shape[1]))
    return _IntegrateFunction.apply((unit.mode, kind, wf, wc, K, act, slot, holder), x1, x2, z1, z2, wparam)


def integrate_list(unit, x_list):
    """SumIntegration / ConcatenationIntegration over any number of inputs (a chain of launches, the reference's
    order: ((x0 + x1) + x2) ...), the weighted units over two."""
    out = integrate(unit, x_list[0], x_list[1])
    for x in x_list[2:]:
        out = integrate(unit, out, x)
    return out
