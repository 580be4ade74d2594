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

# (din, dh, dout) at the edges of every compile-time class of gshac_mlp2_act / gshac_mlp2_backward, grouped by the forward kernel they reach (the
# backward has the resident-weights classes and its plain kernel: what the forward's wide kernel takes runs the plain backward)
CLASS_EDGES = [
    # <192,40,32>: the class itself, one short in every size, the smallest layer, one output, a ragged hidden tile under a full output tile
    (192, 40, 32), (191, 39, 31), (1, 1, 1), (5, 40, 1), (100, 17, 32),
    # <48,100,240>: the same, with dh = 41 and dout = 33 just past <192,40,32>, and CAT-3DGS's stage MLP
    (48, 100, 240), (47, 99, 239), (1, 41, 1), (48, 41, 33), (20, 100, 60),
    # k_mlp2_mfma_wide<100,176>: one past <192,40,32> and past <96,100,175> in din and in dout, its own limit, one past <48,100,240> in din
    (193, 40, 32), (97, 100, 175), (96, 100, 176), (608, 100, 176), (49, 100, 33),
    # the plain k_mlp2: one past the wide kernel and past <48,100,240> in each size, a small and a tall layer, and 16 (din + dh) floats = 64 KB exactly
    (609, 100, 176), (48, 101, 240), (48, 100, 241), (49, 100, 240), (3, 101, 2), (7, 300, 9), (1, 1023, 1), (1023, 1, 1), (512, 512, 3),
    # 3-5-2 is no layer of the plain kernels, small as it is: din <= 192, dh <= 40 and dout <= 32 put it into <192,40,32>, as that class's layer of a
    # few units.  The plain kernels' small layer is 3-101-2 above (dh = 101 is one past <48,100,240>, and the wide kernel has no backward).
    (3, 5, 2)]
EDGE_KERNELS = ["<192,40,32>"] * 5 + ["<48,100,240>"] * 5 + ["wide"] * 5 + ["plain"] * 9 + ["<192,40,32>"]
OVER_THE_LIMIT = [(1, 1024, 1), (1024, 1, 1)]           # 16 (din + dh) floats = 64 KB + 64 B: refused
EDGE_ROWS = [1, 16, 17, 389]                            # the forward's row counts: a partial tile, a full one, one row more, several blocks
LOOP_ROWS = 32785                                       # 2049 16-row tiles: more than 256 workgroups x 8 waves, the persistent loop's second trip
LOOP_SHAPES = [(20, 30, 30), (20, 100, 60)]             # <192,40,32> and <48,100,240>, narrow (the oracle's CPU time)
# The backward's shapes.  The kink rule below drops a row with P = 1 - (1 - 1.4e-4)^dh: 6.4 % of rows at dh = 512 and 9-15 % at dh = 1023, so the shapes
# with dh > 300 leave and 768-256-5 (about 3.5 %) stands at the size limit instead.
BWD_EDGES = [s for s in CLASS_EDGES if s[1] <= 300] + [(768, 256, 5)]
# ((din, dh, dout), n, slab rows): past n = 65 536 the slabs of the resident-weights classes grow beyond 128 rows, past n = 32 768 the plain kernel's.
# 3-5-2 at 36 869 rows is in <192,40,32> and so still in 128-row slabs, 289 of them; 3-101-2 is the plain kernel's grown-slab case.
GROWN_SLAB = [((20, 30, 30), 73733, 160), ((20, 100, 60), 73733, 160), ((3, 101, 2), 36869, 160), ((3, 5, 2), 36869, 128)]
BITWISE_EDGES = [(47, 99, 239), (191, 39, 31), (3, 101, 2), (3, 5, 2)]      # one padded shape per backward kernel (and 3-5-2, see above)
GUARDED_EDGES = [(47, 99, 239), (191, 39, 31), (97, 100, 175), (3, 101, 2), (3, 5, 2)]
SMALL = 30          # a gradient with fewer elements is held to gamma_bound, not to the maximum error of another float32 program
U = 2.0 ** -24


def edge_act(i):
    """the activation of the backward's i-th shape: the two alternate"""
    return "leaky_relu" if i % 2 else "relu"


def edge_seed(i):
    return 1000 + 10 * i


def grown_seed(j):
    """the seed of GROWN_SLAB[j]; its activation is edge_act(j)"""
    return 5000 + 10 * j


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


def grad_magnitudes(x, w1, b1, w2, b2, dy, act, slope=SLOPE):
    """closed_form_grads on absolute values (float64 in): what each gradient's terms add up to without cancellation.  act' is taken from the
    true h; |act(h)| <= |x| |W1^T| + |b1|."""
    h = x @ w1.T + b1
    G = (dy.abs() @ w2.abs()) * act_grad(h, act, slope)
    H = x.abs() @ w1.abs().T + b1.abs()
    return G @ w1.abs(), G.T @ x.abs(), G.sum(0), dy.abs().T @ H, dy.abs().sum(0)


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) for float32: the relative error bound of k roundings in a row"""
    assert k * U < 1
    return k * U / (1 - k * U)


def gamma_bound(x, w1, b1, w2, b2, dy, act, slope=SLOPE):
    """Elementwise a-priori bounds on |float32 gradient - float64 gradient| for any summation order, given equal activation masks (the
    fixture rule): gamma_k x grad_magnitudes with k = din + dh + dout + n, more than the roundings of the longest chain (dW2: din + 1 for h,
    n for the sum over rows; dW1: dout for dy W2, one each for act' and the product, n for the sum; dx: dout + dh + 2)."""
    n, din = x.shape
    k = din + w1.shape[0] + w2.shape[0] + n
    return [gamma(k) * m for m in grad_magnitudes(x, w1, b1, w2, b2, dy, act, slope)]


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
