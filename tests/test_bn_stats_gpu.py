"""Single-launch BN statistics kernels (bn_fwd_stats / bn_bwd_stats):
float64 reference at every ResNet-50 b64 shape and at edge shapes, bitwise
determinism under uneven load, hipGraph replay, and grid changes on one
module."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from byteps_amd import ops as K  # noqa: E402
from byteps_amd.torch.fused_bn import FusedBNReLU  # noqa: E402

# (N, C, H, W): the 12 distinct BN shapes of ResNet-50 at batch 64
RESNET50_B64 = [
    (64, 64, 112, 112), (64, 256, 56, 56), (64, 128, 56, 56),
    (64, 512, 28, 28), (64, 64, 56, 56), (64, 256, 28, 28),
    (64, 1024, 14, 14), (64, 128, 28, 28), (64, 512, 14, 14),
    (64, 2048, 7, 7), (64, 256, 14, 14), (64, 512, 7, 7),
]
EDGE = [
    (1, 64, 1, 1),      # M = 1
    (5, 2048, 1, 1),    # M = 5 < 16 channel-slice blocks
    (4, 8, 28, 28),     # C = 8
    (2, 2048, 7, 7),    # C = 2048, M = 98
    (3, 40, 9, 11),     # C = 40, odd H×W
]
SHAPES = RESNET50_B64 + EDGE
EPS, MOM = 1e-5, 0.1
RTOL = 1e-4     # fp32 accumulation, relative to the sum of magnitudes


def _x(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    # per-channel offsets so the mean is not ~0
    x = torch.randn(N, C, H, W, generator=g) * 1.5 + \
        torch.linspace(-1.0, 2.0, C).view(1, C, 1, 1)
    return x.to("cuda", torch.bfloat16).contiguous(
        memory_format=torch.channels_last)


class _Stats:
    """Direct calls of the two kernels with their own workspace/counters."""

    def __init__(self, M, C):
        core = K.core()
        self.core, self.M, self.C = core, M, C
        n = max(core.bn_stats_ws(M, C, 0), core.bn_stats_ws(M, C, 1))
        self.ws = torch.empty(n, device="cuda")
        self.tickets = torch.zeros(2 * core.BN_TICKET_WORDS,
                                   dtype=torch.int32, device="cuda")

    def fwd(self, x2d, rm=None, rv=None):
        C = self.C
        mean = torch.empty(C, device="cuda")
        invstd = torch.empty(C, device="cuda")
        upd = rm is not None
        if not upd:
            rm = torch.zeros(C, device="cuda")
            rv = torch.ones(C, device="cuda")
        self.core.bn_fwd_stats(
            x2d.data_ptr(), self.M, C, EPS, MOM, mean.data_ptr(),
            invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), int(upd),
            self.ws.data_ptr(), self.tickets.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        return mean, invstd

    def bwd(self, x2d, dy2d, mask, mean, invstd):
        sums2 = torch.empty(2 * self.C, device="cuda")
        self.core.bn_bwd_stats(
            x2d.data_ptr(), dy2d.data_ptr(),
            mask.data_ptr() if mask is not None else 0, self.M, self.C,
            mean.data_ptr(), invstd.data_ptr(), sums2.data_ptr(),
            int(mask is not None), self.ws.data_ptr(),
            self.tickets.data_ptr() + 4 * self.core.BN_TICKET_WORDS,
            torch.cuda.current_stream().cuda_stream)
        return sums2


def _flat(x):
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N * H * W, C)


def _close(got, ref, scale, rtol=RTOL):
    err = (got.double() - ref).abs()
    bound = rtol * scale + 1e-30
    assert bool((err <= bound).all()), \
        "max err/bound %.3g" % (err / bound).max().item()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fwd_stats_vs_float64(shape):
    N, C, H, W = shape
    M = N * H * W
    x = _x(N, C, H, W, seed=C + M)
    m = FusedBNReLU(C, relu=True).cuda().train()
    x2 = _flat(x).double()
    mean64 = x2.mean(0)
    var64 = x2.var(0, unbiased=False)
    unb64 = x2.var(0, unbiased=True) if M > 1 else var64

    mean, invstd = _Stats(M, C).fwd(_flat(x))
    _close(mean, mean64, x2.abs().mean(0))
    # var = E[x²] - mean²: its fp32 error is relative to E[x²]
    ref_invstd = (var64 + EPS).rsqrt()
    ex2 = (x2 * x2).mean(0)
    _close(invstd, ref_invstd, ref_invstd * ex2 / (var64 + EPS))

    # running stats: one update per call, through the module
    rm, rv = torch.zeros(C, dtype=torch.float64, device="cuda"), \
        torch.ones(C, dtype=torch.float64, device="cuda")
    for _ in range(2):
        m(x)
        rm = rm + MOM * (mean64 - rm)
        rv = rv + MOM * (unb64 - rv)
        torch.cuda.synchronize()
        _close(m.running_mean, rm, x2.abs().mean(0))
        _close(m.running_var, rv, rv.abs() + ex2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [True, False])
def test_bwd_stats_vs_float64(shape, relu):
    N, C, H, W = shape
    M = N * H * W
    x = _x(N, C, H, W, seed=C + M).requires_grad_(True)
    m = FusedBNReLU(C, relu=relu).cuda().train()
    with torch.no_grad():
        m.bias.uniform_(-0.5, 0.5)      # a mask that is not ~half by symmetry
    y = m(x)
    g = torch.Generator().manual_seed(M)
    dy = torch.randn(N, C, H, W, generator=g).to("cuda", torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    y.backward(dy)
    torch.cuda.synchronize()

    x2 = _flat(x.detach()).double()
    mean64 = x2.mean(0)
    xhat = (x2 - mean64) * (x2.var(0, unbiased=False) + EPS).rsqrt()
    dz = _flat(dy).double()
    if relu:
        dz = dz * (_flat(y.detach()) > 0).double()
    _close(m.bias.grad, dz.sum(0), dz.abs().sum(0))
    # fp32 mean/invstd move xhat by ~1e-7 relative; far inside RTOL
    _close(m.weight.grad, (dz * xhat).sum(0), (dz * xhat).abs().sum(0))


def _stream_load(big):
    """A long streaming kernel on a second stream (uneven load)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(4):
            big.mul_(1.0001)
    return side


@pytest.mark.parametrize("shape", [(64, 64, 112, 112), (64, 2048, 7, 7),
                                   (64, 256, 14, 14), (3, 40, 9, 11)],
                         ids=lambda s: "x".join(map(str, s)))
def test_stats_bitwise_deterministic(shape):
    N, C, H, W = shape
    M = N * H * W
    xa = _flat(_x(N, C, H, W, seed=1)).contiguous()
    xb = _flat(_x(N, C, H, W, seed=2)).contiguous()
    dy = _flat(_x(N, C, H, W, seed=3)).contiguous()
    mask = torch.randint(0, 256, (M * C // 8,), dtype=torch.uint8,
                         device="cuda")

    def run(st, x):
        mean, invstd = st.fwd(x)
        return mean, invstd, st.bwd(x, dy, mask, mean, invstd), \
            st.bwd(x, dy, None, mean, invstd)

    ref_a = run(_Stats(M, C), xa)
    ref_b = run(_Stats(M, C), xb)

    st = _Stats(M, C)
    big = torch.empty(64 << 20, device="cuda").fill_(1.0)
    for i in range(6):
        # alternate inputs on one workspace: the reducers' partial lines
        # were read with other values by the previous call
        x, ref = (xa, ref_a) if i % 2 == 0 else (xb, ref_b)
        side = _stream_load(big) if i >= 2 else None
        got = run(st, x)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for g_, r_ in zip(got, ref):
            assert torch.equal(g_, r_), "call %d differs" % i
    # every launch leaves its counters at zero
    assert int(st.tickets.abs().sum().item()) == 0


def _fwd_bwd(m, x, res, dy):
    y = m(x, res)
    gx, gres, gw, gb = torch.autograd.grad(y, (x, res, m.weight, m.bias), dy)
    return y, gx, gres, gw, gb


def test_hipgraph_replay_matches_eager():
    N, C, H, W = 32, 256, 14, 14
    m = FusedBNReLU(C, relu=True).cuda().train()
    with torch.no_grad():
        m.weight.uniform_(0.5, 1.5)
        m.bias.uniform_(-0.5, 0.5)
    x = _x(N, C, H, W, 11).requires_grad_(True)
    res = _x(N, C, H, W, 12).requires_grad_(True)
    dy = _x(N, C, H, W, 13)

    # warm up on a side stream (allocates the module's counters), then
    # start the eager copy from the same state
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fwd_bwd(m, x, res, dy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m_eager = copy.deepcopy(m)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _fwd_bwd(m, x, res, dy)
    # capture does not run the kernels: running stats are untouched
    torch.cuda.synchronize()
    assert torch.equal(m.running_mean, m_eager.running_mean)

    for step in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        want = _fwd_bwd(m_eager, x, res, dy)
        torch.cuda.synchronize()
        for i, (g_, w_) in enumerate(zip(got, want)):
            assert torch.equal(g_, w_), "replay %d output %d" % (step, i)
        assert torch.equal(m.running_mean, m_eager.running_mean)
        assert torch.equal(m.running_var, m_eager.running_var)


def test_grid_change_on_one_module():
    C = 64
    shapes = [(64, C, 56, 56), (2, C, 8, 8)]   # two-level fold vs one block
    m = FusedBNReLU(C, relu=True).cuda().train()
    inputs = [(_x(*s, seed=i).requires_grad_(True), _x(*s, seed=10 + i))
              for i, s in enumerate(shapes)]
    want = []
    for x, dy in inputs:            # each on a fresh module
        f = FusedBNReLU(C, relu=True).cuda().train()
        y = f(x)
        gx, = torch.autograd.grad(y, (x,), dy)
        want.append((y, gx))
    for rep in range(4):
        k = rep % 2
        x, dy = inputs[k]
        y = m(x)
        gx, = torch.autograd.grad(y, (x,), dy)
        torch.cuda.synchronize()
        assert torch.equal(y, want[k][0]), "call %d forward" % rep
        assert torch.equal(gx, want[k][1]), "call %d backward" % rep
