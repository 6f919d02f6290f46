"""The encoder's image half with ovm_tune_set gdino_enc_fold = 1 against today's sequence (knob 0) on the same weights and image.

Knob 1: the position term of the sampling-offsets | attention-weights projection is a per-plan table P = pos W_off^T + b_off, the
value and offsets projections are one GEMM over [value | offw] whose epilogue adds P to the columns n >= d_model (GemmParams::r_n0),
and the split rows three GEMMs read are written by their producers (the out-projection's epilogue, the Swin stages' out-norms, the
last layer's final norm) instead of by row passes.

Reduced detectors (the SMALL pattern of test_gpu_gdino_engine.py) on a 120 x 168 image: 315 / 88 / 24 / 6 tokens per level, S = 433,
none a multiple of 128.
  case A  d_model 64, 4 heads: NOW = 192, N = 256 - the residual window starts at column 64, inside a 128-wide tile
  case B  d_model 256, 8 heads, one encoder layer: NOW = 384, N = 640 - the window on a tile boundary, five column tiles
Layer 0's operands come from the test key gdino_enc_tap (copies kept for ovm_gdino_debug_copy; no launch added).

Bounds. Against fp64: 4 x the knob-0 route's own error against the same reference plus one fp32 ulp of the block's largest
|reference| (the convention of tests/test_gpu_roi_glue.py), per column block. Through the engine: boxes 2e-5, logits 1e-4 of their
largest magnitude (test_swin_qkv_projection_inside_the_window_kernel, test_gpu_gdino_mlp_fused.py: the same kind of A/B).
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from common import assert_close
from test_gpu_gdino_engine import SMALL, _engine

pytestmark = pytest.mark.gpu

CASES = {"A": dict(SMALL), "B": dict(SMALL, d_model=256, heads=8, enc_layers=1, ffn_dim=256)}
HW, HW2 = (120, 168), (160, 200)
IDS = [101, 500, 1012, 600, 601, 1012, 102]
MSDA = "model.encoder.layers.0.deformable_layer.self_attn."


@lru_cache(maxsize=None)
def _state_dict(case):
    from ovmono3d_amd.gdino.config import GDinoConfig
    from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict
    return synth_gdino_state_dict(11, GDinoConfig(**CASES[case]), bert_hidden=64, bert_layers=2, bert_ffn=128, vocab=2000)


def _image(hw, seed=31):
    return torch.randint(0, 256, (3,) + hw, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _levels(hw, sd):
    """token counts of the encoder's levels and how many of them the neck projects straight from a Swin stage"""
    nfeat = sum(1 for k in sd if "hidden_states_norms.stage" in k and k.endswith(".weight"))
    h, w = (hw[0] + 3) // 4, (hw[1] + 3) // 4
    sizes = [(h, w)]
    for _ in range(3):
        h, w = (h + 1) // 2, (w + 1) // 2
        sizes.append((h, w))
    lv = sizes[4 - nfeat:]
    lv.append(((lv[-1][0] - 1) // 2 + 1, (lv[-1][1] - 1) // 2 + 1))          # 3 x 3, stride 2, pad 1
    return [a * b for a, b in lv], nfeat


class _knobs:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from ovmono3d_amd import lib
        self.L = lib.load()
        for k, v in self.kv.items():
            assert self.L.ovm_tune_set(k.encode(), v) == 0
        return self.L

    def __exit__(self, *exc):
        for k in self.kv:
            self.L.ovm_tune_set(k.encode(), 0)


@lru_cache(maxsize=None)
def _run(case, knob, device):
    """one eager forward with the taps on: outputs, launch count and layer 0's operands (shared by the tests below, never changed)"""
    device = torch.device(device)
    cfg, sd = CASES[case], _state_dict(case)
    D, NOW = cfg["d_model"], cfg["heads"] * 4 * 4 * 3
    S = sum(_levels(HW, sd)[0])
    with _knobs(gdino_enc_fold=knob, gdino_enc_tap=1):
        eng = _engine(device, sd, cfg, use_graphs=False)
        logits, boxes = eng.forward(_image(HW).to(device), IDS)
    halves = lambda name: eng.debug(name, (S, D // 2), torch.int32).view(torch.int16).cpu()
    out = dict(logits=logits[:, :len(IDS)].cpu(), boxes=boxes.cpu(), launches=eng.launches(), S=S,
               topk=eng.debug("topk", (cfg["num_queries"],), torch.int32).cpu(), pos=eng.debug("enc_pos", (S, D)).cpu(),
               vis=eng.debug("enc_vis0", (S, D)).cpu(), hi=halves("enc_vis0_hi"), lo=halves("enc_vis0_lo"))
    if knob:
        voff = eng.debug("enc_voff0", (S, D + NOW)).cpu()
        out.update(val=voff[:, :D], ow=voff[:, D:], P=eng.debug("enc_P0", (S, NOW)).cpu())
    else:
        out.update(val=eng.debug("enc_val0", (S, D)).cpu(), ow=eng.debug("enc_ow0", (S, NOW)).cpu())
    return out


def _ulp(x):
    return float(np.spacing(np.float32(float(x.abs().max()))))


@pytest.mark.parametrize("case", ["A", "B"])
def test_merged_projection_and_table_against_fp64(device, case):
    sd = _state_dict(case)
    r0, r1 = _run(case, 0, str(device)), _run(case, 1, str(device))
    assert torch.equal(r0["vis"], r1["vis"]) and torch.equal(r0["pos"], r1["pos"])       # the same fp32 rows enter both routes
    w = lambda n: sd[MSDA + n].double()
    Wv, bv = w("value_proj.weight"), w("value_proj.bias")
    Wo = torch.cat([w("sampling_offsets.weight"), w("attention_weights.weight")])
    bo = torch.cat([w("sampling_offsets.bias"), w("attention_weights.bias")])
    vis, pos = r0["vis"].double(), r0["pos"].double()
    ref_val, ref_ow, ref_P = vis @ Wv.t() + bv, (vis + pos) @ Wo.t() + bo, pos @ Wo.t() + bo
    err = lambda got, ref: float((got.double() - ref).abs().max())
    e0_val, e0_ow = err(r0["val"], ref_val), err(r0["ow"], ref_ow)
    e1_val, e1_ow, e_P = err(r1["val"], ref_val), err(r1["ow"], ref_ow), err(r1["P"], ref_P)
    print(f"FIG enc fold {case} vs fp64 (absolute; max|ref| value {float(ref_val.abs().max()):.3e}, offsets {float(ref_ow.abs().max()):.3e}, "
          f"table {float(ref_P.abs().max()):.3e}): value knob0 {e0_val:.3e} knob1 {e1_val:.3e}; offsets knob0 {e0_ow:.3e} "
          f"knob1 {e1_ow:.3e}; table {e_P:.3e}")
    assert e0_val > 0 and e0_ow > 0
    assert e1_val <= 4 * e0_val + _ulp(ref_val), "value columns"
    assert e1_ow <= 4 * e0_ow + _ulp(ref_ow), "offsets | logits columns (residual window)"
    assert e_P <= 4 * e0_ow + _ulp(ref_P), "the plan's table"


@pytest.mark.parametrize("case", ["A", "B"])
def test_out_projection_epilogue_writes_the_row_pass_split(device, case):
    """split_f16 (epilogue) and split_f16_nt (row pass) are the same two conversions, so the rows must agree in every bit"""
    r0, r1 = _run(case, 0, str(device)), _run(case, 1, str(device))
    assert bool((r0["hi"] != 0).any()) and bool((r0["lo"] != 0).any())
    assert torch.equal(r1["hi"], r0["hi"]) and torch.equal(r1["lo"], r0["lo"])
    back = r1["hi"].view(torch.float16).double() + r1["lo"].view(torch.float16).double()
    assert float((back - r1["vis"].double()).abs().max()) <= 2.0 ** -21 * float(r1["vis"].abs().max())


@pytest.mark.parametrize("case", ["A", "B"])
def test_engine_outputs_and_launch_count(device, case):
    cfg, sd = CASES[case], _state_dict(case)
    r0, r1 = _run(case, 0, str(device)), _run(case, 1, str(device))
    nfeat = _levels(HW, sd)[1]
    print(f"FIG enc fold {case}: launches {r0['launches']} -> {r1['launches']} ({nfeat} levels straight from a stage)")
    assert r1["launches"] == r0["launches"] - (2 * cfg["enc_layers"] + nfeat + 1)
    logits, boxes = r1["logits"], r1["boxes"]
    if not torch.equal(r0["topk"], r1["topk"]):
        # a near-tie of the two-stage selection flipped a query: pin knob 1's selection to knob 0's and compare those outputs
        print(f"FIG enc fold {case}: top-k differs in {int((r0['topk'] != r1['topk']).sum())} slots, pinned to knob 0's")
        with _knobs(gdino_enc_fold=1):
            eng = _engine(device, sd, cfg, use_graphs=False)
            eng.set_force_topk(r0["topk"].to(device))
            lg, bx = eng.forward(_image(HW).to(device), IDS)
            logits, boxes = lg[:, :len(IDS)].cpu(), bx.cpu()
    assert torch.isfinite(logits).all() and torch.isfinite(boxes).all()
    d_box, d_log = float((boxes - r0["boxes"]).abs().max()), float((logits - r0["logits"]).abs().max())
    print(f"FIG enc fold {case} knob 1 vs 0: max |d boxes| {d_box:.3e}, max |d logits| {d_log:.3e} (max |logits| {float(r0['logits'].abs().max()):.3e})")
    assert_close(boxes, r0["boxes"], 2e-5, "pred_boxes (knob 1 vs 0)")
    assert_close(logits, r0["logits"], 1e-4, "pred_logits (knob 1 vs 0)")


def test_graph_replay_equals_eager(device):
    r1 = _run("A", 1, str(device))
    img = _image(HW).to(device)
    with _knobs(gdino_enc_fold=1):
        eng = _engine(device, _state_dict("A"), CASES["A"], use_graphs=True)
        first = [t.clone() for t in eng.forward(img, IDS)]                # eager pass, then the capture
        replay = [t.clone() for t in eng.forward(img, IDS)]
    assert torch.equal(first[0][:, :len(IDS)].cpu(), r1["logits"]) and torch.equal(first[1].cpu(), r1["boxes"]), "eager pass differs"
    assert torch.equal(replay[0], first[0]) and torch.equal(replay[1], first[1]), "graph replay differs from the eager pass"


def test_each_plan_owns_its_tables(device):
    cfg, sd = CASES["A"], _state_dict("A")
    a, b = _image(HW).to(device), _image(HW2, 37).to(device)
    res, held = {}, {}
    for knob in (0, 1):
        with _knobs(gdino_enc_fold=knob):
            eng = _engine(device, sd, cfg)
            first = [t.clone() for t in eng.forward(a, IDS)]
            eng.forward(b, IDS)
            third = [t.clone() for t in eng.forward(a, IDS)]
        assert eng.debug_scalar("plans") == 2
        held[knob] = eng.debug_scalar("plan_bytes")
        res[knob] = (first, third)
    first, third = res[1]
    assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])
    tables = sum(cfg["enc_layers"] * sum(_levels(hw, sd)[0]) * cfg["heads"] * 48 * 4 for hw in (HW, HW2))
    print(f"FIG enc fold plan bytes: knob 0 {held[0]}, knob 1 {held[1]} (+{held[1] - held[0]}), tables {tables}")
    assert held[1] - held[0] >= tables


def test_knob_is_bound_to_the_plan(device):
    """the pattern of tests/test_gpu_gdino_plan_knobs.py: a plan built with the knob on keeps its sequence after the knob goes to 0;
    a shape first seen afterwards gets today's sequence"""
    cfg, sd = CASES["A"], _state_dict("A")
    a, b = _image(HW).to(device), _image(HW2, 37).to(device)
    with _knobs(gdino_enc_fold=1) as L:
        eng = _engine(device, sd, cfg, use_graphs=False)
        logits, boxes = (t.clone() for t in eng.forward(a, IDS))
        on = eng.launches()
        assert L.ovm_tune_set(b"gdino_enc_fold", 0) == 0
        logits2, boxes2 = eng.forward(a, IDS)
        assert eng.launches() == on == _run("A", 1, str(device))["launches"]
        assert torch.equal(logits2, logits) and torch.equal(boxes2, boxes)
        eng.forward(b, IDS)
        after = eng.launches()
    fresh = _engine(device, sd, cfg, use_graphs=False)
    fresh.forward(b, IDS)
    print(f"FIG enc fold plan-bound knob: {on} launches kept; new shape {after}, fresh knob-0 engine {fresh.launches()}")
    assert after == fresh.launches()


def test_full_size_once(device):
    """Swin-B / BERT-base / 900 queries at 532 x 532 (S = 6,015, N = 640: 47 x 5 tiles): 12 encoder launches, 3 neck row passes and the
    decoder's row pass go"""
    from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict
    from ovmono3d_amd.gdino.config import GDinoConfig
    from test_gpu_gdino_engine import MEAN, STD
    from ovmono3d_amd.gdino.engine import GdinoEngine
    sd = synth_gdino_state_dict(3)
    img = _image((532, 532), 41).to(device)
    outs = []
    for knob in (0, 1):
        with _knobs(gdino_enc_fold=knob):
            eng = GdinoEngine(device, sd, GDinoConfig(), pixel_mean=MEAN, pixel_std=STD, flip_channels=True, use_graphs=False)
            logits, boxes = eng.forward(img, IDS)
            launches, topk = eng.launches(), eng.debug("topk", (900,), torch.int32).cpu()
            if knob and not torch.equal(topk, outs[0][3]):
                # 900 of 6,015 proposals: a near-tie of the selection flipped; the outputs compared are those of knob 0's selection
                print(f"FIG enc fold full size: top-k differs in {int((topk != outs[0][3]).sum())} slots, pinned to knob 0's")
                eng.set_force_topk(outs[0][3].to(device))
                logits, boxes = eng.forward(img, IDS)
            outs.append((logits[:, :len(IDS)].cpu(), boxes.cpu(), launches, topk))
            del eng
    print(f"FIG enc fold full size: launches {outs[0][2]} -> {outs[1][2]}")
    assert outs[1][2] == outs[0][2] - 16
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    print(f"FIG enc fold full size knob 1 vs 0: max |d boxes| {float((outs[1][1] - outs[0][1]).abs().max()):.3e}, "
          f"max |d logits| {float((outs[1][0] - outs[0][0]).abs().max()):.3e} (max |logits| {float(outs[0][0].abs().max()):.3e})")
    assert_close(outs[1][1], outs[0][1], 2e-5, "pred_boxes (full size, knob 1 vs 0)")
    assert_close(outs[1][0], outs[0][0], 1e-4, "pred_logits (full size, knob 1 vs 0)")
