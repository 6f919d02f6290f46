"""fp64 restatement of the fused GEMM epilogues (csrc/gemm.hpp) and of the implicit-GEMM 3x3 convolution, with the cases, inputs and
the comparison that tests/test_gpu_gemm_epilogues.py runs against ovm_op_gemm_epi.

Everything here is CPU torch. The operands enter as the kernel sees them (`seen`: hi + lo of the fp16 split, hi alone in one-pass
mode), so operand rounding is not part of the error; everything after that is float64. The device layouts are written from their
definitions, not from the C code:

  * every output is described as (flat destination index, value) per logical element (m, n), so C with ldc, X with ldx and row_map,
    the padded-NHWC O, Q / K / V^T and the ConvTranspose image are all checked by one routine (`check`): nothing outside the index set
    may change, nothing inside it may still hold the sentinel, and the values must match (torch.equal in the exact family);
  * V^T token order: bits 2 and 3 of the token index swapped (inside each group of 16 tokens);
  * ConvTranspose 2x2: column n = (a*2 + bb)*Cout + co of row (b, i, j) is pixel (2i + a, 2j + bb), channel co;
  * padded NHWC: row (b, y, x) is pixel (y + 1, x + 1) of a [B][H + 2][W + 2] image;
  * interleaved split image: logical column n has its hi half at il_col(n) = (n // 32)*64 + n % 32 and its lo half 32 further.

`reference(case, inp, precision, mut=...)` can also restate the epilogue WRONGLY in one named way (MUTATIONS);
tests/test_gemm_epi_ref_cpu.py asserts that `check` rejects every applicable mutation of every case, which is the proof that the GPU
tests would fail on a kernel with that defect.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

SENTINEL = 7.5                                   # exact in fp16, and no integer: the exact family cannot produce it
Q_SCALE = float(torch.tensor(0.125 * 1.44269504088896340736, dtype=torch.float32))    # 1/sqrt(64) * log2(e), as fp32
STORE, RESID, GELU, QKV, PATCH, CONVT = 0, 1, 2, 3, 4, 5

MUTATIONS = ("bias_last_group", "gamma_ignored", "r2_dropped", "relu_o_on_c", "resid_before_act", "vt_unpermuted", "q_unscaled",
             "ab_swapped", "border0", "pos_off_by_one", "rowmap_neg_written", "conv_tap_T", "last_row_sentinel")


@dataclass
class Case:
    name: str
    epi: int
    M: int
    N: int
    K: int
    conv: Optional[Tuple[int, int, int, int]] = None      # (B, cH, cW, cC): A is the un-bordered NHWC image, K = 9 cC
    relu: int = 0                                          # STORE: 0 | 1 ReLU | 2 GELU(erf); GELU: 3 = QuickGELU
    ldc: int = 0                                           # STORE: > 0 -> C
    ldr: int = 0                                           # STORE: > 0 -> R
    ldr2: int = 0                                          # STORE: > 0 -> R2
    ldo: int = 0                                           # STORE: > 0 -> O; CONVT: pixel stride (0: Cout)
    relu_o: int = 0
    pad: Optional[Tuple[int, int, int]] = None             # STORE: O is a bordered image, rows are (B, padH, padW)
    o_il: int = 0
    o_off: int = 0                                         # O starts this many elements into the caller's buffer (a column offset)
    gamma: bool = False
    row_map: bool = False
    ldx: int = 0
    B: int = 1
    T: int = 0                                             # QKV / PATCH tokens per image
    Tpad: int = 0
    heads: int = 0
    G2: int = 0
    pos_rows: int = 0
    G: int = 0
    Cout: int = 0
    border: bool = False                                   # CONVT: bordered destination
    seed: int = 0

    @property
    def transcendental(self) -> bool:
        return self.epi == GELU or (self.epi == STORE and self.relu == 2)


def il_col(n):
    return (n // 32) * 64 + n % 32


def vt_token(t):
    """Token order of V^T: bits 2 and 3 of the index swapped."""
    b2, b3 = (t >> 2) & 1, (t >> 3) & 1
    return (t & ~0b1100) | (b2 << 3) | (b3 << 2)


def seen(x: torch.Tensor, precision: int) -> torch.Tensor:
    """The fp32 tensor as the kernel sees it: hi = fp16(x) (+ lo = fp16(x - hi) in split mode), in float64."""
    hi = x.half()
    s = hi.double()
    if precision == 3:
        s = s + (x - hi.float()).half().double()
    return s


def gelu_erf(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_quick(z):
    return z * torch.sigmoid(1.702 * z)


def conv3x3_preact(A, W, conv, tap_transposed=False):
    """A [B][cH][cW][cC], W [N][(dy*3 + dx)*cC + c] (float64) -> [B cH cW][N]: zero padding 1, cross-correlation."""
    B, H, Wd, Cc = conv
    P = torch.zeros(B, H + 2, Wd + 2, Cc, dtype=torch.float64)
    P[:, 1:H + 1, 1:Wd + 1] = A
    Z = torch.zeros(B * H * Wd, W.shape[0], dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            tap = dx * 3 + dy if tap_transposed else dy * 3 + dx
            Z += P[:, dy:dy + H, dx:dx + Wd].reshape(-1, Cc) @ W[:, tap * Cc:(tap + 1) * Cc].T
    return Z


def convt_rows(w):
    """ConvTranspose2d(k 2, s 2) weight [Cin][Cout][2][2] -> GEMM rows [(a*2 + bb)*Cout + co][ci]."""
    Cin, Cout = w.shape[:2]
    return w.permute(2, 3, 1, 0).reshape(4 * Cout, Cin)


def conv_rows(w):
    """Conv2d(k 3) weight [Cout][Cin][3][3] -> GEMM rows [co][(dy*3 + dx)*Cin + ci]."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(case: Case, family: str) -> Dict[str, torch.Tensor]:
    """Seeded fp32 CPU tensors. exact: small integers (gamma a power of two), so every sum is exact in fp32 and in the fp16 split."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    ex = family == "exact"

    def rnd(*shape, lo=-3, hi=3, scale=1.0):
        if ex:
            return torch.randint(lo, hi + 1, shape, generator=g).float()
        return torch.randn(*shape, generator=g) * scale

    M, N, K = case.M, case.N, case.K
    inp = {}
    a_shape = case.conv if case.conv else (M, K)
    inp["A"] = rnd(*a_shape, lo=-1, hi=1)
    inp["W"] = rnd(N, K, lo=-2, hi=2, scale=1.0 / math.sqrt(K))
    inp["bias"] = rnd(case.Cout if case.epi == CONVT else N)
    if case.gamma:
        inp["gamma"] = (2.0 ** torch.randint(1, 3, (N,), generator=g)).float() if ex else torch.rand(N, generator=g) + 0.5
    if case.ldr:
        inp["R"] = rnd(M, case.ldr, lo=-4, hi=4)
    if case.ldr2:
        inp["R2"] = rnd(M, case.ldr2, lo=-4, hi=4)
    if case.epi == RESID:
        inp["X"] = rnd(M, case.ldx, lo=-8, hi=8)
        if case.row_map:
            perm = torch.randperm(M, generator=g)
            drop = torch.rand(M, generator=g) < 0.2
            drop[M - 1] = False                              # the last leftover row stays observable
            inp["row_map"] = torch.where(drop, torch.full((M,), -1), perm).to(torch.int32)
    if case.epi == PATCH:
        inp["X"] = torch.full((case.B * case.T, case.ldx), SENTINEL)
        inp["pos"] = rnd(case.pos_rows, N, lo=-5, hi=5)
    if case.epi == STORE and case.ldc:
        inp["C"] = torch.full((M, case.ldc), SENTINEL)
    if case.epi == STORE and case.ldo:
        rows = case.pad[0] * (case.pad[1] + 2) * (case.pad[2] + 2) if case.pad else M
        inp["O"] = torch.full((rows * case.ldo,), SENTINEL)
    if case.epi == GELU:
        inp["O"] = torch.full((M * case.ldo,), SENTINEL)
    if case.epi == QKV:
        inp["Q"] = torch.full((case.B * case.heads * case.T * 64,), SENTINEL)
        inp["Kout"] = torch.full((case.B * case.heads * case.T * 64,), SENTINEL)
        inp["Vt"] = torch.full((case.B * case.heads * 64 * case.Tpad,), SENTINEL)
    if case.epi == CONVT:
        side = 2 * case.G + (2 if case.border else 0)
        inp["O"] = torch.full((case.B * side * side * (case.ldo or case.Cout),), SENTINEL)
    return inp


# ------------------------------------------------------------------------------------------------ reference
@dataclass
class Out:
    name: str                    # key of the buffer in `inp`
    buf0: torch.Tensor           # initial contents, flat fp32
    idx: torch.Tensor            # [rows][cols] int64 flat destination of every logical element
    val: torch.Tensor            # [rows][cols] float64
    m: torch.Tensor              # [rows] GEMM row of each logical row
    kind: str                    # "f32" | "split"
    il: bool = False             # interleaved split image: hi at idx, lo at idx + 32
    exact: bool = True           # exact family: compare with torch.equal (False: Q, scaled by a non-power of two)
    sentinel: bool = True        # buf0 is sentinel-filled (False: the in-place residual stream)
    e32: float = 0.0             # transcendental epilogues: error of the fp32 torch evaluation against fp64


def _act_err(f, z):
    ref = f(z)
    return float((f(z.float()).double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def reference(case: Case, inp: Dict[str, torch.Tensor], precision: int, mut: Optional[str] = None) -> List[Out]:
    M, N, K = case.M, case.N, case.K
    A, W = seen(inp["A"], precision), seen(inp["W"], precision)
    Z = conv3x3_preact(A, W, case.conv, mut == "conv_tap_T") if case.conv else A @ W.T
    bias = inp["bias"].double()
    ms = torch.arange(M)
    ns = torch.arange(N)
    if case.epi == CONVT:
        bias = bias[ns % case.Cout]
    if mut == "bias_last_group":
        bias = bias.clone()
        bias[(N - 1) // 4 * 4:] = 0.0
    V = Z + bias
    outs: List[Out] = []

    if case.epi == STORE:
        act = {0: lambda z: z, 1: torch.relu, 2: gelu_erf}[case.relu]
        res = torch.zeros_like(V)
        if case.ldr:
            res = res + inp["R"].double()[:, :N]
        if case.ldr2 and mut != "r2_dropped":
            res = res + inp["R2"].double()[:, :N]
        val = act(V + res) if mut == "resid_before_act" else act(V) + res
        e32 = _act_err(gelu_erf, V) if case.relu == 2 else 0.0
        if case.ldc:
            cv = torch.relu(val) if mut == "relu_o_on_c" else val
            outs.append(Out("C", inp["C"].flatten(), ms[:, None] * case.ldc + ns[None, :], cv, ms, "f32", e32=e32))
        if case.ldo:
            rows = ms
            if case.pad:
                Bp, H, Wd = case.pad
                x, y, b = ms % Wd, (ms // Wd) % H, ms // (Wd * H)
                o = 0 if mut == "border0" else 1
                rows = (b * (H + 2) + y + o) * (Wd + 2) + x + o
            ov = torch.relu(val) if case.relu_o else val
            outs.append(Out("O", inp["O"], rows[:, None] * case.ldo + ns[None, :] + case.o_off, ov, ms, "split", e32=e32))
    elif case.epi == RESID:
        gam = inp["gamma"].double() if (case.gamma and mut != "gamma_ignored") else torch.ones(N, dtype=torch.float64)
        rows = inp["row_map"].long() if case.row_map else ms
        if mut == "rowmap_neg_written":
            rows = torch.where(rows < 0, ms, rows)             # the dropped row lands on its own index instead
        keep = rows >= 0
        X0 = inp["X"].double()
        idx = rows[keep][:, None] * case.ldx + ns[None, :]
        if mut == "rowmap_neg_written":
            # two GEMM rows may now hit one X row: accumulate both, as a kernel without the guard would
            X = X0.clone()
            X.view(-1).index_add_(0, idx.flatten(), (gam * V[keep]).flatten())
            val = X.view(-1)[idx]
        else:
            val = X0.view(-1)[idx] + gam * V[keep]
        outs.append(Out("X", inp["X"].flatten(), idx, val, ms[keep], "f32", sentinel=False))
    elif case.epi == GELU:
        f = gelu_quick if case.relu == 3 else gelu_erf
        cols = il_col(ns) if case.o_il else ns
        outs.append(Out("O", inp["O"], ms[:, None] * case.ldo + cols[None, :], f(V), ms, "split", il=bool(case.o_il), e32=_act_err(f, V)))
    elif case.epi == QKV:
        Dm = N // 3
        b, t = ms // case.T, ms % case.T
        for which, name in enumerate(("Q", "Kout", "Vt")):
            f = torch.arange(Dm)
            head, d = f // 64, f % 64
            bh = b[:, None] * case.heads + head[None, :]
            v = V[:, which * Dm:(which + 1) * Dm]
            if which == 0 and mut != "q_unscaled":
                v = v * Q_SCALE
            if which < 2:
                idx = (bh * case.T + t[:, None]) * 64 + d[None, :]
            else:
                tp = t if mut == "vt_unpermuted" else vt_token(t)
                idx = (bh * 64 + d[None, :]) * case.Tpad + tp[:, None]
            outs.append(Out(name, inp[name], idx, v, ms, "split", exact=which != 0))
    elif case.epi == PATCH:
        b, p = ms // case.G2, ms % case.G2
        c0 = case.T - case.G2
        c1 = 1 if c0 > 0 else 0
        prow = p + (0 if mut == "pos_off_by_one" else c1)
        val = V + inp["pos"].double()[prow]
        idx = (b * case.T + c0 + p)[:, None] * case.ldx + ns[None, :]
        outs.append(Out("X", inp["X"].flatten(), idx, val, ms, "f32"))
    elif case.epi == CONVT:
        G, Cout = case.G, case.Cout
        q, co = ns // Cout, ns % Cout
        a, bb = q // 2, q % 2
        if mut == "ab_swapped":
            a, bb = bb, a
        j, i, b = ms % G, (ms // G) % G, ms // (G * G)
        bd = 1 if case.border else 0
        o = 0 if mut == "border0" else bd
        side = 2 * G + 2 * bd
        ps = case.ldo or Cout
        idx = ((b[:, None] * side + 2 * i[:, None] + a[None, :] + o) * side + 2 * j[:, None] + bb[None, :] + o) * ps + co[None, :] + case.o_off
        outs.append(Out("O", inp["O"], idx, V, ms, "split"))
    else:
        raise ValueError(case.epi)
    if mut == "last_row_sentinel":
        for o in outs:
            live = o.m != M - 1
            o.idx, o.val, o.m = o.idx[live], o.val[live], o.m[live]
    return outs


def render(outs: List[Out], precision: int) -> Dict[str, torch.Tensor]:
    """The buffers a device that computed exactly `outs` would hand back (fp32; split outputs as hi + lo, hi alone in one-pass mode)."""
    got = {}
    for o in outs:
        buf = o.buf0.clone()
        v = o.val.float()
        if o.il:
            hi = v.half()
            buf[o.idx.flatten()] = hi.float().flatten()
            buf[o.idx.flatten() + 32] = (v - hi.float()).half().float().flatten()
        elif o.kind == "split" and precision == 1:
            buf[o.idx.flatten()] = v.half().float().flatten()
        else:
            buf[o.idx.flatten()] = v.flatten()
        got[o.name] = buf
    return got


# ------------------------------------------------------------------------------------------------ comparison
def tolerance(case: Case, precision: int, o: Out) -> float:
    """Scale-relative bound (max |got - ref| / max |ref|) of a float-family output.

    precision 3, fp32 destination: the bound test_gemm_store uses, max(2e-6, 3e-8 sqrt(K)) (fp32 accumulation noise); a split fp16
    destination adds the 1e-6 test_split_f16_roundtrip asserts for one split round trip. precision 1: 3e-3, as test_gemm_store.
    A transcendental epilogue differs from the plain one only in the activation, whose slope is <= 1.13 (GELU) / 1.1 (QuickGELU), so it
    keeps that budget and adds an allowance for erff / expf: 4 x the error of the fp32 torch evaluation of the same activation on the
    fp64 pre-activation (the margin the SAM and Depth Pro stage tests use)."""
    if precision == 1:
        t = 3e-3
    else:
        t = max(2e-6, 3e-8 * math.sqrt(case.K)) + (1e-6 if o.kind == "split" else 0.0)
    return t + 4.0 * o.e32


def gather(o: Out, buf: torch.Tensor) -> torch.Tensor:
    flat = buf.flatten().double()
    v = flat[o.idx]
    return v + flat[o.idx + 32] if o.il else v


def check(case: Case, family: str, precision: int, got: Dict[str, torch.Tensor], ref: List[Out], report=None):
    """Asserts that the device buffers `got` are what `ref` describes. `report(name, err, tol)` receives every float figure."""
    for o in ref:
        buf = got[o.name].detach().cpu().flatten().float()
        assert buf.numel() == o.buf0.numel(), f"{case.name}/{o.name}: buffer size"
        mask = torch.zeros(buf.numel(), dtype=torch.bool)
        mask[o.idx.flatten()] = True
        if o.il:
            mask[o.idx.flatten() + 32] = True
        assert int(mask.sum()) == o.idx.numel() * (2 if o.il else 1), f"{case.name}/{o.name}: reference index map is not one-to-one"
        outside = ~mask
        # bit for bit: view the fp32 words as integers
        same = buf.view(torch.int32)[outside] == o.buf0.view(torch.int32)[outside]
        assert bool(same.all()), (f"{case.name}/{o.name}: {int((~same).sum())} elements outside the output range changed "
                                  f"(first flat index {int(torch.nonzero(outside)[~same][0])})")
        if o.sentinel:
            left = buf[mask] == SENTINEL
            assert not bool(left.any()), (f"{case.name}/{o.name}: {int(left.sum())} in-range elements still hold the sentinel "
                                          f"(first flat index {int(torch.nonzero(mask)[left][0])})")
        g = gather(o, buf)
        if family == "exact" and o.exact and not case.transcendental:
            bad = g != o.val
            assert not bool(bad.any()), (f"{case.name}/{o.name}: {int(bad.sum())} elements differ from the exact reference, first at "
                                         f"logical {tuple(int(v) for v in torch.nonzero(bad)[0])}")
        else:
            err = float((g - o.val).abs().max() / o.val.abs().max().clamp_min(1e-30))
            tol = tolerance(case, precision, o)
            if report:
                report(o.name, err, tol)
            assert err <= tol, f"{case.name}/{o.name}: scale-relative error {err:.3e} > {tol:.2e}"


def mutations_for(case: Case) -> List[str]:
    """The mutations that change what this case's epilogue computes."""
    m = ["bias_last_group", "last_row_sentinel"]
    if case.conv:
        m.append("conv_tap_T")
    if case.epi == STORE:
        if case.ldr2:
            m.append("r2_dropped")
        if case.relu_o and case.ldc:
            m.append("relu_o_on_c")
        if case.ldr and case.relu:
            m.append("resid_before_act")
        if case.pad and case.ldo:
            m.append("border0")
    if case.epi == RESID:
        if case.gamma:
            m.append("gamma_ignored")
        if case.row_map:
            m.append("rowmap_neg_written")
    if case.epi == QKV:
        m += ["vt_unpermuted", "q_unscaled"]
    if case.epi == PATCH and case.T > case.G2:
        m.append("pos_off_by_one")
    if case.epi == CONVT:
        m.append("ab_swapped")
        if case.border:
            m.append("border0")
    return m


# ------------------------------------------------------------------------------------------------ cases
# Shapes: the smallest that reach each path of launch_prec / launch_ws / launch_one / launch256 (see the table in
# tests/test_gpu_gemm_epilogues.py). name -> (M, N, K, rows as (B, H, W) for the padded-NHWC destination)
SHAPES = {
    "ragged": (200, 100, 128, (1, 10, 20)),      # partial M tile, partial N tile (N % 4 == 0)
    "tail": (132, 192, 128, (1, 3, 44)),         # 4 leftover rows
    "splitk": (130, 128, 1024, (1, 10, 13)),     # ksplit = 4 at f16x3 (K = 2048 at f16: SPLITK_K_F16), leftover path off
    "g256": (260, 256, 64, (2, 10, 13)),         # 256-tile kernel, 4 leftover rows
    "g256sk": (260, 256, 512, (2, 10, 13)),      # ... with split-K hint 2
}
SPLITK_K_F16 = 2048
CONV_SHAPES = {
    "conv": (1, 3, 44, 64, 72),                  # (B, cH, cW, cC, N): M = 132 -> tiles + 4 leftover rows, K = 576
    "convsk": (1, 12, 12, 128, 64),              # M = 144, K = 1152: 36 k-steps of 32 -> ksplit = 4 at f16x3, slices cross taps
}


def _store(name, shape, M, N, K, rows, variant, conv=None, seed=0):
    if variant == "plain":        # no activation; C with ldc > N; planar O with a pixel stride
        return Case(f"store_plain/{shape}", STORE, M, N, K, conv=conv, ldc=N + 3, ldo=N + 8, seed=seed)
    if variant == "relu_r":       # ReLU, one residual
        return Case(f"store_relu_r/{shape}", STORE, M, N, K, conv=conv, relu=1, ldc=N + 3, ldr=N + 4, seed=seed)
    if variant == "full":         # every flag: ReLU, R + R2 with their own strides, C keeps the sign, O relu'd into a bordered image
        return Case(f"store_full/{shape}", STORE, M, N, K, conv=conv, relu=1, ldc=N + 3, ldr=N + 4, ldr2=N + 8, ldo=N + 4, relu_o=1,
                    pad=rows, seed=seed)
    if variant == "gelu":
        return Case(f"store_gelu/{shape}", STORE, M, N, K, conv=conv, relu=2, ldc=N, ldr=N, ldo=N, seed=seed)
    raise ValueError(variant)


def build_cases() -> List[Case]:
    cs: List[Case] = []
    s = 0
    for shape, (M, N, K, rows) in SHAPES.items():
        for v in ("plain", "relu_r", "full", "gelu"):
            s += 1
            cs.append(_store(v, shape, M, N, K, rows, v, seed=s))
        for gamma, rmap in ((True, True), (False, False)):
            s += 1
            cs.append(Case(f"resid_{'gamma_map' if gamma else 'plain'}/{shape}", RESID, M, N, K, gamma=gamma, row_map=rmap, ldx=N + 4, seed=s))
        for relu in (0, 3):
            for o_il in (0, 1):
                if o_il and N % 32:
                    continue                                 # an interleaved image has whole 32-column groups
                s += 1
                cs.append(Case(f"gelu_{'quick' if relu == 3 else 'erf'}{'_il' if o_il else ''}/{shape}", GELU, M, N, K, relu=relu,
                               ldo=2 * N if o_il else N, o_il=o_il, seed=s))
    for shape, (B, H, Wd, Cc, N) in CONV_SHAPES.items():
        for v in ("plain", "relu_r", "full", "gelu"):
            s += 1
            cs.append(_store(v, shape, B * H * Wd, N, 9 * Cc, (B, H, Wd), v, conv=(B, H, Wd, Cc), seed=s))
    s += 1
    cs.append(Case("qkv/qkv", QKV, 260, 768, 64, B=2, T=130, Tpad=192, heads=4, seed=s))
    for shape, (M, N, K, _) in (("ragged", SHAPES["ragged"]), ("tail", SHAPES["tail"])):
        G2 = M // 2
        for lead in (0, 1, 5):                               # none | class | class + 4 register tokens
            s += 1
            cs.append(Case(f"patch_lead{lead}/{shape}", PATCH, M, N, K, B=2, T=lead + G2, G2=G2, pos_rows=G2 + (1 if lead else 0),
                           ldx=N + 4, seed=s))
    for name, B, G, ldo, off, border in (("convt_plain/convt", 2, 9, 0, 0, False), ("convt_border/convt", 2, 9, 0, 0, True),
                                         ("convt_stride/convt", 2, 9, 48, 16, False), ("convt_stride_border/convt", 2, 9, 48, 16, True),
                                         ("convt_border/convt_tail", 33, 2, 48, 16, True)):
        s += 1
        cs.append(Case(name, CONVT, B * G * G, 128, 64, B=B, G=G, Cout=32, ldo=ldo, o_off=off, border=border, seed=s))
    return cs


CASES = build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def families(case: Case) -> List[str]:
    return ["float"] if case.transcendental else ["exact", "float"]


def with_k(case: Case, K: int) -> Case:
    """The same case at another reduction length (split-K needs K = 2048 in one-pass mode)."""
    from dataclasses import replace
    return replace(case, K=K, name=f"{case.name}@K{K}")
