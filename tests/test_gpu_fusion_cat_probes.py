"""The split-input conv mode of mmt_gemm on the MI355X (RGBT_Fusion_Cat's first conv: the 3x3 conv of the channel
concat of two NHWC maps, read in place through a / a1 / k_split), with exact integer operands, NaN-poisoned storage
around every buffer and torch.equal-style comparison of whole storage images (tests/fusion_cat_probes.py).

Shapes: map sides 3 (every pixel a corner, an edge or the centre) and 5, B = 2 packed and with an image pitch larger
than the map, channel splits (8, 8), (64, 64), (64, 128) and (72, 56) -- the last off the LDS-DMA kernel's 64-element
K step, which the register-staged kernel runs -- N in {8, 72, 136}, fp32 / bf16 / fp16, each kernel forced through
`impl` where it takes the shape."""
import pytest
import torch

import fusion_cat_probes as P

pytestmark = pytest.mark.gpu

SWEEP = [(d, i) for d in ("bf16", "fp16") for i in P.IMPLS] + [("f32", 0)]


def _run(s):
    t = P.storage(s, "cuda")
    st = P.launch(s, t)
    assert st == 0, (s, st)
    return t["c"]


@pytest.mark.parametrize("dname,impl", SWEEP)
def test_split_conv_matches_integer_reference(dname, impl):
    """Every shape the named kernel takes, in the runtime's two forms (16-bit C with bias + ReLU; plain fp32 C):
    the whole C image equals the reference, guard elements untouched, no NaN read in; and the k_split = 0 launch of
    the same kernel on the materialised concat is bitwise the same image."""
    cases = P.sweep(dname, impl)
    assert cases, "no shape reaches impl %d in %s" % (impl, dname)
    kernels = set()
    for s in cases:
        kernels.add(P.kernel_of(s))
        got = _run(s)
        assert P.same(got, P.expected_image(s)), s
        one = s.but(split=False)
        if P.takes(one):
            assert torch.equal(_run(one).view(torch.uint8), got.view(torch.uint8)), s
    if impl > 0 and dname != "f32":
        assert kernels == {("glds", impl)}
    if impl == -1 or dname == "f32":
        assert kernels == {("reg",)}
    if impl == 0 and dname != "f32":
        assert kernels == {("reg",), ("glds", 3)}  # auto: the off-step splits on the register-staged kernel


def test_off_step_split_runs_the_register_staged_kernel():
    """(72, 56): mmt_gemm_select names the register-staged kernel for 16-bit operands too; that launch is probed."""
    for dname in ("bf16", "fp16"):
        for N in P.NS:
            s = P.Spec(5, 72, 56, N, dtype=dname, pitched=True, act=2, bias=True, c_f32=0)
            assert P.kernel_of(s) == ("reg",)
            assert P.same(_run(s), P.expected_image(s)), s


def _selector_cases(h, ks, c1):
    centre = (h // 2) * h + h // 2
    pixels = {"corner": 0, "far corner": h * h - 1, "edge": h // 2, "centre": centre}
    for src in (0, 1):
        n = c1 if src else ks
        for ch in (0, n - 1):
            for nm, pix in pixels.items():
                yield src, pix, ch, nm


@pytest.mark.parametrize("dname,impl", [("bf16", 0), ("bf16", -1), ("bf16", 1), ("bf16", 2), ("fp16", 3), ("fp16", 4),
                                        ("f32", 0)])
def test_selector_one_hot_reproduces_the_taps(dname, impl):
    """One pixel, one channel, one source set to 1: every output pixel that sees it through a tap reproduces that
    tap's weights of that channel exactly, everything else is zero -- both sources, first and last channel of each,
    a corner, the far corner, an edge and the centre pixel, in both images."""
    ran = 0
    for h in P.SIDES:
        for ks, c1 in P.SPLITS:
            for src, pix, ch, nm in _selector_cases(h, ks, c1):
                s = P.Spec(h, ks, c1, 72, dtype=dname, impl=impl, pitched=bool(pix & 1), fill=(src, pix, ch))
                if not P.takes(s):
                    continue
                ran += 1
                got = _run(s)
                assert torch.equal(P.reference(s), P.one_hot_expected(s))  # the two references agree
                assert P.same(got, P.expected_image(s)), (s, nm)
                assert float(got[:s.M, :s.N].abs().sum()) > 0
    assert ran >= 2 * 2 * 4 * 4  # at least the on-step (or, register-staged, all) splits of both sides


@pytest.mark.parametrize("dname,impl", [("bf16", 0), ("bf16", -1), ("fp16", 1), ("bf16", 2), ("bf16", 3), ("fp16", 4),
                                        ("f32", 0)])
def test_census_all_ones_counts_every_tap_inside_the_map(dname, impl):
    """Both maps all ones, weights distinct small integers: each output is the sum of the weights of the taps that
    fall inside the map over all channels of both sources (a tap or a channel chunk dropped, doubled or read from
    the wrong map changes it)."""
    ran = 0
    for h in P.SIDES:
        for pitched in (False, True):
            for ks, c1 in P.SPLITS:
                for N in P.NS:
                    s = P.Spec(h, ks, c1, N, dtype=dname, impl=impl, pitched=pitched, fill="ones")
                    if not P.takes(s):
                        continue
                    ran += 1
                    _, W, _ = P.operands(P._key(s))
                    # written out: pixel (y, x) sums the taps (ky, kx) with (y + ky - 1, x + kx - 1) inside
                    wsum = W.sum(3).double()  # [N][3][3]
                    exp = torch.zeros(s.h, s.h, N, dtype=torch.float64)
                    for y in range(h):
                        for x in range(h):
                            for ky in range(3):
                                for kx in range(3):
                                    if 0 <= y + ky - 1 < h and 0 <= x + kx - 1 < h:
                                        exp[y, x] += wsum[:, ky, kx]
                    assert torch.equal(P.reference(s), exp.view(1, h * h, N).expand(s.B, -1, -1).reshape(s.M, N))
                    assert P.same(_run(s), P.expected_image(s)), s
    assert ran >= 12


@pytest.mark.parametrize("name", list(P.bad_specs()))
@pytest.mark.parametrize("dname", ["bf16", "f32"])
def test_unbuilt_combinations_return_ebadarg_and_launch_nothing(name, dname):
    s, over = P.bad_specs()[name]
    s = s.but(dtype=dname)
    t = P.storage(s, "cuda")
    assert P.launch(s, t, **over) == P.EBADARG
    assert bool(torch.isnan(t["c"]).all())  # C as it was filled: nothing ran
