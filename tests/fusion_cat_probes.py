"""Probe inputs and exact integer references of the split-input conv mode of mmt_gemm (no tests here): the 3x3
implicit-GEMM conv whose input is the channel concatenation of two NHWC maps, read in place (mmt_gemm_params.a /
a1 / k_split with conv_h > 0; RGBT_Fusion_Cat's first conv).  In the manner of tests/gemm_probes.py:

Operands are small integers, exact in bf16, fp16 and fp32, and every partial sum stays below 2^24, so the kernels'
fp32 accumulation is exact in any order, tile shape or K split, and the expected output is one rounding of an exact
value.  The reference is the conv of the materialised concat in float64 (F.conv2d on the CPU).

Poisoned storage: both maps are stored with pixel stride lda = max(k_split, cin - k_split) + 8, the channels past a
map's own count NaN; `pitched` puts NaN rows between the images (image pitch > h * h pixels) and every buffer ends in
8 NaN rows; C has ldc = N + 8 and 8 rows past M, pre-filled with NaN.  The kernels clamp padding taps and rows past M
to in-bounds pixels and zero them, so the surplus is never part of the contract; `same` compares whole storage images.
"""
import ctypes
import dataclasses
import functools

import torch
import torch.nn.functional as F

NAN = float("nan")
PAD = 8
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SPLITS = ((8, 8), (64, 64), (64, 128), (72, 56))  # (k_split, cin - k_split); the last is off the LDS-DMA K step
SIDES = (3, 5)
NS = (8, 72, 136)
EBADARG = -10000


@dataclasses.dataclass(frozen=True)
class Spec:
    h: int            # map side (conv_h)
    ks: int           # channels of the first map (k_split)
    c1: int           # channels of the second map
    N: int
    dtype: str = "bf16"
    impl: int = 0
    B: int = 2
    pitched: bool = False
    act: int = 0
    bias: bool = False
    c_f32: int = 1
    k3: int = 1
    up: int = 1
    split: bool = True    # False: one launch on the materialised concat, k_split = 0
    fill: str = "rand"    # rand | ones | (source, pixel, channel) one-hot
    seed: int = 0

    def but(self, **kw):
        return dataclasses.replace(self, **kw)

    @property
    def cin(self):
        return self.ks + self.c1

    @property
    def M(self):
        return self.B * self.h * self.h

    @property
    def K(self):
        return (9 if self.k3 else 1) * self.cin

    @property
    def pitch(self):
        hw = self.h * self.h
        return (hw + 7) // 8 * 8 + 8 if self.pitched else hw

    @property
    def lda(self):
        return (max(self.ks, self.c1) if self.split else self.cin) + PAD


def _lib():
    from mmt_amd import _lib
    return _lib


def dtype_code(dname):
    L = _lib()
    return {"f32": L.MMT_F32, "bf16": L.MMT_BF16, "fp16": L.MMT_F16}[dname]


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(s):
    """(X [B][h][h][cin], W [N][3][3][cin], bias [N]) as int64 CPU tensors (shared by the split and the concat
    launch of a shape: split / impl / dtype do not enter)."""
    g = torch.Generator().manual_seed(1000 + s.seed)
    vals = torch.tensor([-3, -2, -1, 1, 2, 3])
    taps = 9 if s.k3 else 1
    if s.fill == "rand":
        X = vals[torch.randint(0, 6, (s.B, s.h, s.h, s.cin), generator=g)]
        W = vals[torch.randint(0, 6, (s.N, taps, s.cin), generator=g)]
    else:
        # distinct small integers: neighbouring taps, channels and output columns all differ; <= 251, exact in bf16
        n, t, c = torch.meshgrid(torch.arange(s.N), torch.arange(taps), torch.arange(s.cin), indexing="ij")
        W = 1 + (n * 31 + t * 7 + c * 3) % 251
        if s.fill == "ones":
            X = torch.ones(s.B, s.h, s.h, s.cin, dtype=torch.int64)
        else:
            src, pix, ch = s.fill
            X = torch.zeros(s.B, s.h, s.h, s.cin, dtype=torch.int64)
            X.view(s.B, s.h * s.h, s.cin)[:, pix, ch + (s.ks if src else 0)] = 1
    bias = torch.randint(-8, 9, (s.N,), generator=g) if s.bias else torch.zeros(s.N, dtype=torch.int64)
    return X, W.view(s.N, 3 if s.k3 else 1, 3 if s.k3 else 1, s.cin), bias


def _key(s):  # what the operands and the reference depend on
    return s.but(dtype="bf16", impl=0, split=True, pitched=False, c_f32=1)


@functools.lru_cache(maxsize=None)
def _reference(s):
    X, W, bias = operands(s)
    y = F.conv2d(X.permute(0, 3, 1, 2).double(), W.permute(0, 3, 1, 2).double(), padding=1 if s.k3 else 0)
    y = y.permute(0, 2, 3, 1).reshape(s.M, s.N) + bias.double()
    return y.clamp(min=0) if s.act == 2 else y


def reference(s):
    """[M][N] float64, exact."""
    return _reference(_key(s))


def expected_image(s):
    """The whole C storage image: the reference rounded once to the output type inside M x N, NaN elsewhere."""
    out = torch.full((s.M + PAD, s.N + PAD), NAN, dtype=torch.float32 if s.c_f32 else DT[s.dtype])
    out[:s.M, :s.N] = reference(s).float().to(out.dtype)
    return out


def one_hot_expected(s):
    """The selector probe's expectation written out, independent of F.conv2d: output pixel q sees the one-hot
    pixel p through tap (py - y + 1, px - x + 1) when that is a tap, and the weight of that tap and channel comes
    out; zero elsewhere."""
    src, pix, ch = s.fill
    _, W, _ = operands(_key(s))
    py, px = divmod(pix, s.h)
    out = torch.zeros(s.B, s.h, s.h, s.N, dtype=torch.float64)
    for y in range(s.h):
        for x in range(s.h):
            ky, kx = py - y + 1, px - x + 1
            if 0 <= ky < 3 and 0 <= kx < 3:
                out[:, y, x] = W[:, ky, kx, ch + (s.ks if src else 0)].double()
    return out.view(s.M, s.N)


# ------------------------------------------------------------------------------------------------ storage + launch
def _map_storage(x, lda, pitch, dt):
    """x [B][h*h][c] -> [B * pitch + PAD][lda] with NaN in every element that is not x's."""
    B, hw, c = x.shape
    st = torch.full((B * pitch + PAD, lda), NAN, dtype=dt)
    st[:B * pitch].view(B, pitch, lda)[:, :hw, :c] = x.to(dt)
    return st


def storage(s, device="cpu"):
    """name -> tensor of the launch's buffers (CPU or device)."""
    X, W, bias = operands(_key(s))
    dt = DT[s.dtype]
    Xf = X.view(s.B, s.h * s.h, s.cin)
    t = {}
    if s.split:
        t["a"] = _map_storage(Xf[..., :s.ks], s.lda, s.pitch, dt)
        t["a1"] = _map_storage(Xf[..., s.ks:], s.lda, s.pitch, dt)
    else:
        t["a"] = _map_storage(Xf, s.lda, s.pitch, dt)
    w = torch.full((s.N + PAD, s.K), NAN, dtype=dt)
    w[:s.N] = W.reshape(s.N, s.K).to(dt)
    t["w"] = w
    b = torch.full((s.N + PAD,), NAN, dtype=torch.float32)
    b[:s.N] = bias.float()
    t["bias"] = b
    t["c"] = torch.full((s.M + PAD, s.N + PAD), NAN, dtype=torch.float32 if s.c_f32 else dt)
    return {k: v.to(device) for k, v in t.items()}


_FAKE = 1 << 20  # a non-null 16-byte aligned address the selection never dereferences


def params_of(s, t=None, **over):
    """mmt_gemm_params of a spec; t: storage() on the device (None: fake addresses, for mmt_gemm_select)."""
    L = _lib()
    p = L.GemmParams()
    ptr = (lambda k: _FAKE) if t is None else (lambda k: t[k].data_ptr())
    p.a[0], p.w[0], p.c[0] = ptr("a"), ptr("w"), ptr("c")
    p.a1[0] = ptr("a1") if s.split else None
    p.bias[0] = ptr("bias") if s.bias else None
    p.lda, p.ldc = s.lda, s.N + PAD
    p.a_seg_rows, p.a_segs_a, p.a_stride_a, p.a_stride_b = s.M, 1, (s.pitch if s.pitched else 0), 0
    p.M, p.N, p.K, p.k_split = s.M, s.N, s.K, (s.ks if s.split else 0)
    p.act, p.c_f32, p.groups, p.impl = s.act, s.c_f32, 1, s.impl
    p.conv_h, p.conv_up, p.conv_cin, p.conv_k3 = s.h, s.up, s.cin, s.k3
    for k, v in over.items():
        if k == "a1":
            p.a1[0] = ptr("a1") + 2 if v == "odd" else v
        else:
            setattr(p, k, v)
    return p


def select(s, **over):
    return _lib().gemm_select(params_of(s, **over), dtype_code(s.dtype))


def kernel_of(s):
    """("glds", cfg) / ("reg",) or None (rejected): the library's own answer, no GPU needed."""
    c, L = select(s), _lib()
    if c is None:
        return None
    return ("glds", c.cfg) if c.family == L.GEMM_LDS_DMA else ("reg",)


def takes(s):
    """The kernel s.impl names runs the spec: -1 and fp32 the register-staged tiles, 1.. that LDS-DMA tile, 0 any."""
    k = kernel_of(s)
    if k is None:
        return False
    if s.impl == -1 or s.dtype == "f32":
        return k == ("reg",)
    return True if s.impl == 0 else k == ("glds", s.impl)


def launch(s, t, **over):
    """mmt_gemm on device storage t; returns the status (0, or EBADARG)."""
    import torch as _t
    p = params_of(s, t, **over)
    st = _lib().LIB.mmt_gemm(ctypes.byref(p), dtype_code(s.dtype), _t.cuda.current_stream().cuda_stream)
    _t.cuda.synchronize()
    return st


def same(a, b):
    """Equal storage images, NaN == NaN."""
    a, b = a.float().cpu(), b.float().cpu()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ------------------------------------------------------------------------------------------------ case lists
IMPLS = (0, -1, 1, 2, 3, 4)


def shapes():
    """(h, pitched, ks, c1, N): every side x image pitch x split x N."""
    return [(h, pitched, ks, c1, N) for h in SIDES for pitched in (False, True) for ks, c1 in SPLITS for N in NS]


def sweep(dname, impl):
    """The specs of one (dtype, impl) the named kernel takes (possibly none): the runtime's two forms, 16-bit C with
    bias + ReLU and fp32 C plain."""
    out = []
    for i, (h, pitched, ks, c1, N) in enumerate(shapes()):
        for kw in (dict(act=2, bias=True, c_f32=0 if dname != "f32" else 1), dict()):
            s = Spec(h, ks, c1, N, dtype=dname, impl=impl, pitched=pitched, seed=i, **kw)
            if takes(s):
                out.append(s)
    return out


def bad_specs():
    """name -> (spec, params overrides): every combination the split does not build; each must be MMT_EBADARG."""
    s = Spec(3, 64, 64, 8)
    return {
        "conv_up 2": (s.but(h=4, up=2), {}),  # (a 4 x 4 output map of a 2 x 2 input: valid without the split)
        "conv_k3 2 (flipped taps)": (s.but(k3=2), {}),
        "a1 null": (s, dict(a1=None)),
        "a1 not 16-byte aligned": (s, dict(a1="odd")),
        "k_split % 8": (s, dict(k_split=60)),
        "k_split == conv_cin": (s, dict(k_split=128)),
        "k_split > conv_cin": (s, dict(k_split=136)),
    }
