"""The 8-phase main loop of the 256x256x64 tile (bs_gemm tile 9) against the one-barrier-per-K-tile loop it replaces.

Both loops give every accumulator the same products in the same order, so the comparison is `torch.equal` on every output
buffer, never a tolerance: tile = 9 is the dispatcher's choice, tile = 3209 (ablation bit 32) forces the old loop.  The cases
cover the short K paths (1, 2, 3 K tiles), ragged M, the tail split, convolutions (padding, ReLU on load, stride 2), the FP8
correction stages with each of their per-tile cut-offs, and the backbone's three output forms.  One case per kernel class is
also launched 50 times over: a schedule whose waits are placed right gives the same bits every time.
Every test here needs a real MI355X: run with `pytest -m gpu`."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

OLD_LOOP = 3200          # ablation bit 32 in the hundreds of the tile id
DT = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def L():
    from bodyslam_amd import _lib
    _lib.init(0)
    return _lib


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def f8_rows(L, x, dtype):
    """fp32 [M, K] -> [M, 2K] rows of (hi16 | hi8 | lo8), written by the library's own cast."""
    M, K = x.shape
    out = torch.empty(M, 2 * K, device=dev(), dtype=dtype)
    L.cast_split(x, out, M, K, f8=True)
    return out


def f8_pixels(L, x, dtype):
    """fp32 NHWC -> (hi16 | hi8 | lo8) pixels: the torch statement of the operand format."""
    hi = x.to(dtype)
    lo = x - hi.float()
    hi8 = (x * 2.0 ** L.F8_ACT_HI_EXP).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    lo8 = (lo * 2.0 ** L.F8_ACT_LO_EXP).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    C2 = x.shape[-1] * 2
    return torch.cat([hi.contiguous().view(torch.uint8).view(*x.shape[:-1], C2), hi8, lo8], -1).contiguous().view(dtype)


def run(L, case, tile):
    """case = (A, W, make_outputs, kwargs_of(outputs)); returns the output buffers after one launch with `tile`."""
    A, W, make_outputs, kwargs = case
    outs = make_outputs()
    L.gemm(A, W, outs[0], tile=tile, **kwargs(outs))
    torch.cuda.synchronize()
    return outs


def same_bits(L, case):
    d = L.make_gemm_desc(case[0], case[1], case[2]()[0], tile=9, **case[3](case[2]()))
    assert L.load_library().bs_gemm_tile(L.C.byref(d)) == 9            # the schedule is not a tile id
    new, old = run(L, case, 9), run(L, case, 9 + OLD_LOOP)
    for a, b in zip(new, old):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------------------------ cases
def plain_case(dtype, M, N, K, res=False):
    A = rnd(M, K, seed=1, dtype=dtype)
    W = rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=dtype)
    bias = rnd(N, seed=3)
    r0 = rnd(M, N, seed=4) if res else None

    def outs():
        return [r0.clone() if res else torch.zeros(M, N, device=dev())]

    def kw(o):
        k = dict(M=M, N=N, K=K, lda=K, bias=bias)
        if res:
            k.update(res=o[0], ldr=N)
        return k
    return A, W, outs, kw


def conv_case(L, dtype, B, H, Wd, Cin, Cout, stride, relu_a):
    x = rnd(B, H, Wd, Cin, seed=1, dtype=dtype)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=1 / math.sqrt(9 * Cin), dtype=dtype)
    wk = L.conv_weight(w.permute(0, 2, 3, 1))
    g = L.conv_geom(H, Wd, Cin, 3, 3, stride, 1)
    Ho, Wo = g[3], g[4]
    bias = rnd(Cout, seed=3)
    res = rnd(B, Ho, Wo, Cout, seed=4, dtype=dtype)

    def outs():
        return [torch.zeros(B, Ho, Wo, Cout, device=dev(), dtype=dtype)]

    def kw(o):
        return dict(M=B * Ho * Wo, N=Cout, K=9 * Cin, lda=Cin, conv=g, relu_a=relu_a, bias=bias, res=res, ldr=Cout)
    return x, wk, outs, kw


def f8_plain_case(L, dtype, M, N, K, **extra):
    A8 = f8_rows(L, rnd(M, K, seed=1), dtype)
    W8, (sb0, sb1) = L.f8_weight(rnd(N, K, seed=2, scale=1 / math.sqrt(K)).cpu(), dtype)
    W8 = W8.to(dev())
    bias = rnd(N, seed=3)
    base = dict(M=M, N=N, K=K, lda=2 * K, f8_seg=2 * K, f8_scales=(127 - L.F8_ACT_HI_EXP, sb0, 127 - L.F8_ACT_LO_EXP, sb1), bias=bias)
    base.update(extra)

    def outs():
        return [torch.zeros(M, N, device=dev())]

    def kw(o):
        return base
    return A8, W8, outs, kw


def f8_conv_case(L):
    dtype = torch.float16
    B, H, Wd, C, Co = 2, 20, 24, 128, 256
    x8 = f8_pixels(L, rnd(B, H, Wd, C, seed=1), dtype)
    r8 = f8_pixels(L, rnd(B, H, Wd, Co, seed=3), dtype)
    w = rnd(Co, C, 3, 3, seed=2, scale=1 / math.sqrt(9 * C))
    W8, (sb0, sb1) = L.f8_conv_weight(w.permute(0, 2, 3, 1), dtype)
    W8 = W8.to(dev())
    g = L.conv_geom(H, Wd, C, 3, 3, 1, 1)

    def outs():
        return [torch.zeros(B, H, Wd, 2 * Co, device=dev(), dtype=dtype)]

    def kw(o):
        return dict(M=B * H * Wd, N=Co, K=9 * C, lda=2 * C, conv=g, f8_seg=2 * C, f8_scales=(127 - L.F8_ACT_HI_EXP, sb0, 127 - L.F8_ACT_LO_EXP, sb1),
                    res=r8, ldr=2 * Co, res_f8=True, ldo=2 * Co, out_split_off=Co, out_f8=(L.F8_ACT_HI_EXP, L.F8_ACT_LO_EXP))
    return x8, W8, outs, kw


NB, S, SP, HID = 2, 769, 832, 1024        # the backbone's token geometry at a small batch: 256 cls / padding rows + NB x 768 patch rows


def backbone_case(L, form):
    dtype = torch.float16
    N, K = {"res": (HID, HID), "res_k4096": (HID, 4 * HID), "gelu_planes": (4 * HID, HID), "qkv": (3 * HID, HID)}[form]
    MT = 256 + NB * 768
    A8 = f8_rows(L, rnd(MT, K, seed=1), dtype)
    W8, (sb0, sb1) = L.f8_weight(rnd(N, K, seed=2, scale=1 / math.sqrt(K)).cpu(), dtype)
    W8 = W8.to(dev())
    bias, b2 = rnd(N, seed=3), rnd(NB, N, seed=5)
    base = dict(M=MT, N=N, K=K, lda=2 * K, f8_seg=2 * K, f8_scales=(127 - L.F8_ACT_HI_EXP, sb0, 127 - L.F8_ACT_LO_EXP, sb1), bias=bias,
                f8_skip_from=256, bias2=(b2, 256, 768))
    if form.startswith("res"):
        r0, lam = rnd(MT, N, seed=4), rnd(N, seed=6)

        def outs():
            return [r0.clone()]

        def kw(o):
            return dict(base, scale=lam, res=o[0], ldr=N)
    elif form == "gelu_planes":
        def outs():
            return [torch.zeros(MT, 2 * N, device=dev(), dtype=dtype)]

        def kw(o):
            return dict(base, act=L.ACT_GELU, ldo=2 * N, out_split_off=N, out_f8=(L.F8_ACT_HI_EXP, L.F8_ACT_LO_EXP), out_lo8_rows=256,
                        out_planes_rows=256)
    else:
        def outs():
            return [torch.zeros(NB, 16, SP, 64, device=dev(), dtype=dtype), torch.zeros(NB, 16, SP, 64, device=dev(), dtype=dtype),
                    torch.zeros(NB, 16, 64, SP, device=dev(), dtype=dtype)]

        def kw(o):
            return dict(base, qkv=(HID, S, SP, 0.18, o[1], o[2], True, NB, 256))
    return A8, W8, outs, kw


# ------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 1024, 4096])
def test_plain_same_bits(L, dtype, K):
    same_bits(L, plain_case(dtype, 256 * 3 + 1, 512, K))           # ragged M: one row in the last tile row


def test_tail_split_same_bits(L):
    same_bits(L, plain_case(torch.float16, 256 * 128 + 128, 1024, 4096, res=True))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("stride,relu_a", [(1, False), (1, True), (2, False)])
def test_conv_same_bits(L, dtype, stride, relu_a):
    same_bits(L, conv_case(L, dtype, 2, 24, 32, 256, 256, stride, relu_a))      # 256 -> 256 channels: the chunk / tap walk wraps


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("extra", [dict(), dict(f8_wonly_from=256), dict(f8_skip_from=-1), dict(f8_skip_from=256)],
                         ids=["both", "wonly_from_256", "skip_all", "skip_from_256"])
def test_f8_plain_same_bits(L, dtype, extra):
    same_bits(L, f8_plain_case(L, dtype, 256 * 4, 512, 256, **extra))


def test_f8_conv_same_bits(L):
    same_bits(L, f8_conv_case(L))


@pytest.mark.parametrize("form", ["res", "res_k4096", "gelu_planes", "qkv"])
def test_backbone_forms_same_bits(L, form):
    same_bits(L, backbone_case(L, form))


# ------------------------------------------------------------------------------------------------ rerun determinism
@pytest.mark.parametrize("cls", ["plain", "conv", "f8_plain", "f8_conv"])
def test_rerun_gives_the_same_bits(L, cls):
    case = {"plain": lambda: plain_case(torch.float16, 256 * 16 + 1, 1024, 1024),
            "conv": lambda: conv_case(L, torch.float16, 2, 48, 64, 256, 256, 1, True),
            "f8_plain": lambda: backbone_case(L, "res"),
            "f8_conv": lambda: f8_conv_case(L)}[cls]()
    first = run(L, case, 9)
    for _ in range(49):
        again = run(L, case, 9)
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
