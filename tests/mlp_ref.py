"""float64 restatement of gauspcc_amd.mlp's contract: y = W2 act(W1 x + b1) + b2 and its closed-form gradients, and the fixtures the
CPU and GPU tests share.

Fixture rule: a row with a hidden unit whose float64 |h| < KINK_EPS is left out beforehand, so that the activation masks of a float32 and
a float64 evaluation agree (h is a sum of ~din products of O(1/sqrt(din)) terms; float32 rounding moves it by ~1e-6).  For N(0, 1) inputs and
U(+-1/sqrt(din)) weights, h is about N(0, 1/3): P(|h| < 1e-4) = 1.4e-4 per unit, so about 1.4 % of rows at dh = 100 and 0.6 % at dh = 40."""
import torch

KINK_EPS = 1e-4
SLOPE = 0.01

# (din, dh, dout, act): HAC's mlp_grid; HAC++'s mlp_grid (two output widths); two of its channel-context MLPs; the tiny variant's first; TC-GS's
# mlp_triplane (the plain kernel)
SHAPES = [(96, 100, 175, "relu"), (48, 100, 195, "relu"), (48, 100, 225, "relu"), (150, 40, 30, "leaky_relu"), (190, 40, 30, "leaky_relu"),
          (10, 30, 30, "leaky_relu"), (603, 100, 175, "relu")]


def row_counts(S):
    """a partial tile, a tile edge, a slab edge, several slabs with a ragged last one (S: the implementation's slab size)"""
    return [1, 15, 17, S - 1, S + 1, 3 * S + 5]


def act_fn(h, act, slope=SLOPE):
    return torch.where(h > 0, h, h * (slope if act == "leaky_relu" else 0.0))


def act_grad(h, act, slope=SLOPE):
    return torch.where(h > 0, torch.ones_like(h), torch.full_like(h, slope if act == "leaky_relu" else 0.0))


def forward(x, w1, b1, w2, b2, act, slope=SLOPE):
    return act_fn(x @ w1.T + b1, act, slope) @ w2.T + b2


def closed_form_grads(x, w1, b1, w2, b2, dy, act, slope=SLOPE):
    """(dx, dW1, db1, dW2, db2) of sum(y * dy)"""
    h = x @ w1.T + b1
    g = (dy @ w2) * act_grad(h, act, slope)
    return g @ w1, g.T @ x, g.sum(0), dy.T @ act_fn(h, act, slope), dy.sum(0)


def weights(din, dh, dout, seed):
    """nn.Linear's default range, U(+-1/sqrt(fan_in)), float32"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape, fan: (torch.rand(*shape, generator=g) * 2 - 1) / fan ** 0.5
    return u(dh, din, fan=din), u(dh, fan=din), u(dout, dh, fan=dh), u(dout, fan=dh)


def fixture(din, dh, dout, n, seed):
    """(x, dy, (w1, b1, w2, b2), dropped fraction): n float32 rows that pass the fixture rule, drawn with a margin and cut to n"""
    w = weights(din, dh, dout, seed)
    g = torch.Generator().manual_seed(seed + 1)
    m = n + max(64, n // 8)
    x = torch.randn(m, din, generator=g)
    keep = ((x.double() @ w[0].double().T + w[1].double()).abs() >= KINK_EPS).all(dim=1)
    dropped = 1.0 - float(keep.double().mean())
    x = x[keep][:n].contiguous()
    assert x.shape[0] == n, "margin too small"
    dy = torch.randn(n, dout, generator=g)
    return x, dy, w, dropped
