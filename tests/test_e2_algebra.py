"""The node-local form of the entity first-layer backward (phase E2 of the step kernel), on
the CPU in float64, against the pair-grid definition and against the oracle's autograd
gradient of the 100 slots dW1[0:4], db1 of mlp_entity_B1.  No GPU.

Pair grid (model_2.py:165-170 backward): z_ij = u_i + v_j + a_ij d for i != j with
u = x w0 + (w2 + b1), v = x w1, d = w3 - w2, and dz_ij = [z_ij > 0](rho_i + rho_j), rho_n the
gradient that reaches node n's pair sums.  S0 = sum x_i dz, S1 = sum x_j dz, S2 = sum dz,
S3 = sum a dz; dW1 = (S0, S1, S2 - S3, S3), db1 = S2.

Node-local: the rho_j half summed by columns, so node n contributes rho_n times rho-free
brackets over its row set R_n = {j != n : z_nj > 0} and column set C_n = {i != n : z_in > 0}.
Each bracket is a count and a sum of x over a prefix or suffix of the x-sorted order (the
a = 0 sets), the self pair removed once per side, plus the a = 1 corrections over the node's
row and column neighbours.  a is asymmetric here: a swapped list or x role does not pass.
"""
import numpy as np
import pytest

from hdgnn.data import CommitBatch
from hdgnn.synth import synth_commits
from oracle import model_ref

HS = 20


def pair_grid(x, a, W1, b1, rho):
    ne = len(x)
    off = ~np.eye(ne, dtype=bool)
    S = np.zeros((4, HS))
    for k in range(HS):
        w0, w1, w2, w3 = W1[:, k]
        z = (x * w0 + (w2 + b1[k]))[:, None] + (x * w1)[None, :] + a * (w3 - w2)
        dz = ((z > 0) & off) * (rho[:, k][:, None] + rho[:, k][None, :])
        S[0, k] = (x[:, None] * dz).sum()
        S[1, k] = (x[None, :] * dz).sum()
        S[2, k] = dz.sum()
        S[3, k] = (a * dz).sum()
    return S


def _sorted_set(mask_sorted, grows, csum):
    """count and sum x of a set that is a suffix (grows) or prefix of the sorted order"""
    n = len(mask_sorted)
    c = int(mask_sorted.sum())
    if grows:
        assert mask_sorted[n - c:].all()
        return c, csum[n] - csum[n - c]
    assert mask_sorted[:c].all()
    return c, csum[c]


def node_local(x, a, W1, b1, rho):
    ne = len(x)
    xs = np.sort(x, kind="stable")
    csum = np.concatenate([[0.0], np.cumsum(xs)])
    rows = [np.flatnonzero(a[n]) for n in range(ne)]          # j with a_nj = 1
    cols = [np.flatnonzero(a[:, n]) for n in range(ne)]       # i with a_in = 1
    S = np.zeros((4, HS))
    for k in range(HS):
        w0, w1, w2, w3 = W1[:, k]
        c0, d = w2 + b1[k], w3 - w2
        u, v = x * w0 + c0, x * w1
        for n in range(ne):
            nr, sxr = _sorted_set(u[n] + xs * w1 > 0, w1 >= 0, csum)
            nc, sxc = _sorted_set((xs * w0 + c0) + v[n] > 0, w0 >= 0, csum)
            if u[n] + v[n] > 0:                  # the self pair, in both sets
                nr, nc, sxr, sxc = nr - 1, nc - 1, sxr - x[n], sxc - x[n]
            b = np.array([x[n] * nr + sxc, sxr + x[n] * nc, nr + nc, 0.0])
            for j in rows[n]:
                z0 = u[n] + v[j]
                m0, m1 = float(z0 > 0), float(z0 + d > 0)
                b += (m1 - m0) * np.array([x[n], x[j], 1.0, 0.0])
                b[3] += m1
            for i in cols[n]:
                z0 = u[i] + v[n]
                m0, m1 = float(z0 > 0), float(z0 + d > 0)
                b += (m1 - m0) * np.array([x[i], x[n], 1.0, 0.0])
                b[3] += m1
            S[:, k] += rho[n, k] * b
    return S


def _inputs(ne, seed, real):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(ne) * 3 if real else rng.integers(0, 10, ne).astype(np.float64)
    a = (rng.random((ne, ne)) < 0.3) & ~np.eye(ne, dtype=bool)
    if ne > 2:
        assert (a != a.T).any()
    W1 = rng.standard_normal((4, HS)) * 0.3
    W1[:, 0] = np.abs(W1[:, 0])                  # every prefix / suffix combination of the
    W1[:2, 1] = -np.abs(W1[:2, 1])               # row and column sets occurs
    W1[0, 2], W1[1, 2] = abs(W1[0, 2]), -abs(W1[1, 2])
    W1[0, 3], W1[1, 3] = -abs(W1[0, 3]), abs(W1[1, 3])
    W1[3, 4] = W1[2, 4]                          # d = 0
    b1 = rng.standard_normal(HS) * 0.5
    rho = rng.standard_normal((ne, HS))
    return x, a.astype(np.float64), W1, b1, rho


@pytest.mark.parametrize("real", [False, True], ids=["int_x", "real_x"])
@pytest.mark.parametrize("ne", [2, 7, 33])
def test_node_local_equals_pair_grid(ne, real):
    x, a, W1, b1, rho = _inputs(ne, 40 + ne, real)
    ref = pair_grid(x, a, W1, b1, rho)
    got = node_local(x, a, W1, b1, rho)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("ne", [2, 7, 33])
def test_node_local_equals_oracle_autograd(ne, monkeypatch):
    """rho from the oracle's own graph (the gradient at the first _row_col_sum's output, times
    W5^T), the 100 slots from its autograd; the L2 term of train_loss is taken off"""
    nc = 5
    cb = synth_commits(1, ne, nc, 60 + ne)
    rng = np.random.default_rng(ne)
    a = ((rng.random((1, ne, ne)) < 0.3) & ~np.eye(ne, dtype=bool)[None]).astype(np.uint8)
    cb = CommitBatch(cb.x, a, cb.y, cb.hid, cb.nlen)
    params = model_ref.init_params(70 + ne)
    params["E1.b1"] = (rng.standard_normal(HS) * 0.3).astype(np.float32)
    # x' = relu(o) alive on every node, so a gradient reaches the entity stage (at the zero
    # initial biases a small graph can have o <= 0 throughout)
    params["E3.b1"] = np.full_like(params["E3.b1"], 0.2)
    params["E3.b2"] = np.full_like(params["E3.b2"], 0.5)
    params["E3.w2"] = np.abs(params["E3.w2"])    # o = h w2' + b2' > 0 whatever h >= 0 is
    kept = []
    orig = model_ref._row_col_sum

    def keep(vals, I, J, n):
        out = orig(vals, I, J, n)
        if not kept:                             # the entity aggregate comes first
            out.retain_grad()
            kept.append(out)
        return out

    monkeypatch.setattr(model_ref, "_row_col_sum", keep)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    _, grads = model_ref.loss_and_grads(p64, cb.x.astype(np.float64), cb.a, cb.y, cb.hid, cb.nlen)
    assert kept[0].shape == (1, ne, HS)
    W1, b1, W5 = p64["E1.w1"], p64["E1.b1"], p64["E1.w5"]
    rho = kept[0].grad.numpy()[0] @ W5.T
    S = node_local(cb.x[0].astype(np.float64), a[0].astype(np.float64), W1, b1, rho)
    dW1 = np.stack([S[0], S[1], S[2] - S[3], S[3]])
    g_w1 = grads["E1.w1"] - 0.001 * W1
    g_b1 = grads["E1.b1"] - 0.001 * b1
    scale = max(np.abs(g_w1).max(), np.abs(g_b1).max())
    assert scale > 0
    np.testing.assert_allclose(dW1, g_w1, rtol=0, atol=1e-10 * scale)
    np.testing.assert_allclose(S[2], g_b1, rtol=0, atol=1e-10 * scale)
