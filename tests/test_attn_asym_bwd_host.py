"""The cross-modal backward probes of tests/attn_asym_bwd_probes.py, checked on the CPU: the fp64 reference agrees
with autograd through attn_probes.mam_ref, the census dout is exact in bf16 and leaves dK = 0, every single
attending (sequence, query) of every key weighs >= 4x the GPU bar of dV, four wrong references (a query group
dropped, read from the wrong sequence, cut short, or leaked into a straddling tile's search keys) each break that
bar, and the bars of the random-row comparison are 4x the CPU emulation's worst row."""
import pytest
import torch

import attn_asym_bwd_probes as A
import attn_probes as P
from attn_probes import BM, HEADS, SHAPES

S, H, C = A.S, HEADS, HEADS * 64
DV_BAR = 2.0 ** -7


def _rows(n_t, n_s):
    """(sequence, token) of the S ntok flattened rows."""
    ntok = n_t + n_s
    i = torch.arange(S * ntok)
    return i // ntok, i % ntok


def test_ref_matches_autograd_through_mam_ref():
    n_t, n_s = 17, 45
    qkv, dout = A.random_case(n_t, n_s)
    x = qkv.double().requires_grad_()
    out, _ = P.mam_ref(x, n_t, BM, H, 1)
    out.backward(dout.double())
    got, bound = A.mam_asym_bwd_ref(qkv, dout, n_t)
    assert (got - x.grad).abs().max().item() <= 1e-10
    assert (bound >= 0).all()


@pytest.mark.parametrize("n_t,n_s", SHAPES)
def test_census_is_exact(n_t, n_s):
    """dout survives bf16, the fp64 dK is exactly 0 and dV is W^T dout (P is uniform: q = 0)."""
    qkv, dout, ref, _ = A.census_case(n_t, n_s)
    assert torch.equal(dout.bfloat16().float(), dout)
    assert torch.equal(qkv.bfloat16().float(), qkv)
    _, dk, dv = ref.split(C, -1)
    assert bool((dk == 0).all())
    assert (dv - A.census_dv(A.attend_weights(n_t, n_s), dout)).abs().max().item() <= 1e-9 * dv.abs().max().item()
    # the weights differ between any two sequences at every query
    w = torch.stack([A.census_weight(s, torch.arange(n_t + n_s), n_t, n_s) for s in range(S)])
    assert all((w[a] != w[b]).all() for a in range(S) for b in range(a))


@pytest.mark.parametrize("n_t,n_s", SHAPES)
def test_every_query_shows_in_dv(n_t, n_s):
    """The smallest share of one attending (sequence, query) in its dV entry is >= 4x the 2^-7 relative bar."""
    _, dout, ref, _ = A.census_case(n_t, n_s)
    W = A.attend_weights(n_t, n_s)
    sq, q = _rows(n_t, n_s)
    wq = torch.stack([A.census_weight(s, torch.arange(n_t + n_s), n_t, n_s) for s in range(S)]).reshape(-1).double()
    share = W * wq[:, None]  # [query][key]: what the query adds to dV[key, head, q % 64]
    dv = ref[..., 2 * C:2 * C + 64].reshape(-1, 64)  # head 0 (every head has the same dout)
    entry = dv[:, q % 64].t()  # [query][key]
    ratio = torch.where(W > 0, share / (DV_BAR * entry.abs()), float("inf"))
    print("smallest single-query share of a dV entry: %.1fx the bar" % ratio.min().item())
    assert ratio.min().item() >= 4.0


def _wrong_weights(kind, n_t, n_s):
    """W of a kernel with one mistake in its query groups (P stays 1 / n_q: the forward's lse is right)."""
    ntok = n_t + n_s
    W = A.attend_weights(n_t, n_s)
    sq, q = _rows(n_t, n_s)
    sk, k = sq, q
    search_q, tmpl_k = q >= n_t, k < n_t
    tir_q = search_q & (sq >= BM)
    if kind == "tir_left_out":  # the TIR search queries left out of the template keys' sums
        W[tir_q[:, None] & tmpl_k[None, :]] = 0
    elif kind == "rgb_twice":  # the RGB search queries counted twice in place of the TIR ones
        W[tir_q[:, None] & tmpl_k[None, :]] = 0
        W[(search_q & (sq < BM))[:, None] & tmpl_k[None, :]] *= 2
    elif kind == "last_query":  # the last query of each group removed
        W[(q == n_t - 1) | (q == ntok - 1)] = 0
    elif kind == "straddle_leak":  # search keys of a straddling tile also take the other sequence's search queries
        edge = (n_t + 63) // 64 * 64
        leak_k = (k >= n_t) & (k < edge)
        other = (sq[:, None] % BM == sk[None, :] % BM) & (sq[:, None] != sk[None, :])
        W[search_q[:, None] & leak_k[None, :] & other] = 1.0 / (2 * n_t + n_s)
    return W


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("kind", ["tir_left_out", "rgb_twice", "last_query", "straddle_leak"])
def test_wrong_references_break_the_dv_bar(kind, n_t, n_s):
    """Every key whose attending set the edit changes has a dV channel outside the GPU bar."""
    _, dout, ref, _ = A.census_case(n_t, n_s)
    W, Wx = A.attend_weights(n_t, n_s), _wrong_weights(kind, n_t, n_s)
    changed = (W != Wx).any(0)
    if kind == "straddle_leak":
        assert bool(changed.any()) == (n_t % 64 != 0)
    else:
        assert changed.any()
    dv, dvx = ref[..., 2 * C:], A.census_dv(Wx, dout)
    broken = ((dvx - dv).abs() > DV_BAR * dv.abs()).reshape(-1, C).any(1)
    assert bool((broken == changed).all()), (int(changed.sum()), int((broken & changed).sum()))


def test_random_row_bars_are_four_times_the_emulation():
    worst = torch.zeros(3, dtype=torch.float64)
    for n_t, n_s in P.BWD_RANDOM_SHAPES:
        qkv, dout, ref, _ = A.random_ref(n_t, n_s)
        worst = torch.maximum(worst, P.row_rel_err(A.mam_asym_bwd_emul(qkv, dout, n_t), ref, C))
    print("emulation worst rows: dQ %.5f dK %.5f dV %.5f" % tuple(worst.tolist()))
    for w, e, bar in zip(worst.tolist(), A.ASYM_BWD_ROW_EMUL, A.ASYM_BWD_ROW_BAR):
        assert abs(w - e) <= 0.05 * e, (w, e)
        assert bar == 4 * e
