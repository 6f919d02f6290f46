"""GPU: the depth prompt computed by Depth Pro on the device (ovmono3d_amd/data/depth_prompt.py) through the data mapper, the model,
the one-call path (ovm_infer_depth) and the two entry points. Sizes: tests/depth_prompt_cases.py (tiny main model, TINY Depth Pro, two
images of both orientations, a ResizeShortestEdge that changes the size)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from common import ROOT, assert_close, build_clip_cfg, oracle_params
import depth_prompt_cases as cases

pytestmark = pytest.mark.gpu

CATS = ["chair", "dining table", "sofa"]


@pytest.fixture(scope="module")
def depthpro(device):
    """The TINY Depth Pro with its seeded weights, at build_depthpro's default precision, as the entry points build it."""
    from ovmono3d_amd.data.depth_prompt import build_depth_prompt
    return build_depth_prompt(cases.DEPTHPRO_SPEC, "estimate", cases.DEPTHPRO_CONFIG_JSON, None, device).depthpro


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    folder = tmp_path_factory.mktemp("depth_prompt_images")
    return cases.dataset_dicts(str(folder), cases.write_images(str(folder)))


def _model(cfg, device, seed=cases.MODEL_SEED, drop=()):
    from ovmono3d_amd.modeling import build_model
    from ovmono3d_amd.util.synth_weights import synth_state_dict
    name = cfg.MODEL.CLIP.ARCH if cfg.MODEL.BACKBONE.NAME == "build_clip_backbone" else cfg.MODEL.DINO.MODEL_NAME
    sd = synth_state_dict(name, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, seed=seed)
    model = build_model(cfg, device=device)
    model.load_state_dict({k: v for k, v in sd.items() if not any(d in k for d in drop)})
    return model, sd


def test_inline_equals_files(device, depthpro, images, tmp_path):
    """A mapper whose depth comes from Depth Pro (and is dumped on the way) against a second mapper reading the dumped files: the same
    record["depth"] bit for bit, on the device, and the same detections in every field."""
    from ovmono3d_amd.data import DatasetMapper3D
    from ovmono3d_amd.data.depth_prompt import DepthProPrompt
    cfg = cases.model_cfg()
    inline = DatasetMapper3D(cfg, False, depth_source=DepthProPrompt(depthpro, dump_dir=str(tmp_path / "test")))
    files = DatasetMapper3D(cfg, False, str(tmp_path))
    model, _ = _model(cfg, device)
    for i, d in enumerate(images):
        a = inline(d)
        assert (tmp_path / "test" / (os.path.splitext(os.path.basename(d["file_name"]))[0] + ".npz")).exists()
        b = files(d)
        h, w = cases.HWS[i]
        want = (1, 140, 187) if h < w else (1, 187, 140)
        assert a["depth"].is_cuda and a["depth"].dtype == torch.float32 and tuple(a["depth"].shape) == tuple(b["depth"].shape) == want
        assert torch.equal(a["depth"], b["depth"]) and bool((a["depth"] > 0).all())
        assert torch.equal(a["image"], b["image"])
        out_a = model([a], prompt_depth=torch.stack([a["depth"]]))[0]["instances"]
        out_b = model([b], prompt_depth=torch.stack([b["depth"]]))[0]["instances"]
        cases.assert_instances_equal(out_a, out_b, f"image {i}")


def test_focal_length_modes(device, depthpro, images):
    from ovmono3d_amd.data.depth_prompt import DepthProPrompt
    from ovmono3d_amd.data import read_image
    for i, d in enumerate(images):
        bgr = read_image(d["file_name"], "BGR")
        dev_img = torch.from_numpy(bgr).to(device)
        wide = torch.zeros((bgr.shape[0], bgr.shape[1] + 3, 3), dtype=torch.uint8, device=device)
        wide[:, :bgr.shape[1]] = dev_img
        by_k = DepthProPrompt(depthpro, focal="K")(wide[:, :bgr.shape[1]], "BGR", d["K"])       # a device tensor of any strides
        est = DepthProPrompt(depthpro, focal="estimate")(bgr, "BGR", d["K"])           # a numpy image is uploaded
        assert by_k.is_cuda and tuple(by_k.shape) == tuple(est.shape) == cases.HWS[i]
        assert torch.equal(by_k, depthpro.infer(dev_img, f_px=float(d["K"][0][0]), image_format="BGR")["depth"])
        assert torch.equal(est, depthpro.infer(dev_img, f_px=None, image_format="BGR")["depth"])
        assert not torch.equal(by_k, est)
    with pytest.raises(ValueError):
        DepthProPrompt(depthpro, focal="exif")


def test_new_route_against_the_oracle(device, depthpro, images):
    """The depth the device produced, through prepare_prompt_depth, is what the oracle is given; the model through the mapper's new
    route then matches the oracle within the tolerance of test_gpu_model.py's depth-prompt test (1e-3), and stands off the no-prompt
    run by the margin test_depth_prompt_cpu.py established on the oracle (10 x that): a dropped prompt fails here."""
    from oracle.pipeline import inference
    from ovmono3d_amd.data import DatasetMapper3D
    from ovmono3d_amd.data.depth_prompt import DepthProPrompt, prepare_prompt_depth
    from ovmono3d_amd.data.gpu_resize import DepthPromptResizeGPU
    cfg = cases.model_cfg()
    model, sd = _model(cfg, device)
    mapper = DatasetMapper3D(cfg, False, depth_source=DepthProPrompt(depthpro))
    for i, d in enumerate(images):
        rec = mapper(d)
        raw = depthpro.infer(torch.from_numpy(cases.image_rgb(i)).to(device), image_format="RGB")["depth"]
        prompt = prepare_prompt_depth(raw, cases.HWS[i], DepthPromptResizeGPU(cases.MIN_SIZE, cases.MAX_SIZE))
        assert torch.equal(prompt[None], rec["depth"])
        host = dict(rec, image=rec["image"].cpu())
        assert torch.equal(host["image"], cases.model_input(i, cfg.INPUT.FORMAT)["image"])
        ref = inference(sd, [host], oracle_params(cfg), prompt_depth=prompt.cpu()[None, None])[0]
        out = model([rec], prompt_depth=torch.stack([rec["depth"]]))[0]["instances"]
        assert len(out) == len(ref["scores"]) == 6
        assert torch.equal(out.pred_classes.cpu(), ref["pred_classes"].to(torch.int64))
        got = cases.instances_as_dict(out)
        for f in cases.FIELDS:
            e = assert_close(got[f], ref[f], cases.TOL, f)
            print(f"image {i} {f}: scale-relative error {e:.3e}")
        plain = cases.instances_as_dict(model([rec])[0]["instances"])
        move = cases.max_field_move(got, plain)
        print(f"image {i}: the prompt moves the detections by {move:.3e} (needed: {cases.MARGIN:.1e})")
        assert move >= cases.MARGIN


# ------------------------------------------------------------------------------------------ one call
def _detector(device, cfg):
    from test_gpu_gdino import _small_hf_gdino
    from test_gpu_gdino_engine import SMALL
    from ovmono3d_amd.gdino.config import GDinoConfig
    from ovmono3d_amd.gdino.detector import HashTokenizer, NativeGroundingDino
    hf, _ = _small_hf_gdino()

    class Tok(HashTokenizer):
        def _id(self, w):
            return super()._id(w) % 1900 + 50 if w not in (".", "?") else super()._id(w)
    return NativeGroundingDino(device, hf.state_dict(), Tok(), cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, cfg=GDinoConfig(**SMALL))


def _text_inputs(i, device, cfg):
    d = cases.model_input(i, cfg.INPUT.FORMAT)
    d.pop("oracle2D")
    d["category_list"] = list(CATS)
    d["image"] = d["image"].to(device)
    return [d]


def _prompts(device, depthpro):
    from ovmono3d_amd.data.depth_prompt import prepare_prompt_depth
    from ovmono3d_amd.data.gpu_resize import DepthPromptResizeGPU
    out = []
    for i in range(len(cases.HWS)):
        raw = depthpro.infer(torch.from_numpy(cases.image_rgb(i)).to(device), image_format="RGB")["depth"]
        out.append(prepare_prompt_depth(raw, cases.HWS[i], DepthPromptResizeGPU(cases.MIN_SIZE, cases.MAX_SIZE))[None, None])
    return out


def test_one_call_with_a_depth_prompt_equals_the_staged_path(device, depthpro):
    """ROIHeads3DGDINO with a category_list and a depth prompt: MODEL.AMD.FUSED_INFER True (ovm_infer_depth, one C call) and False (the
    stages sequenced from Python) give the same records bit for bit; the one-call path is really taken, and the prompt really read."""
    prompts = _prompts(device, depthpro)
    outs, fused_calls = [], []
    for fused in (True, False):
        cfg = cases.model_cfg("ROIHeads3DGDINO", extra=["MODEL.AMD.FUSED_INFER", fused])
        model, _ = _model(cfg, device, seed=3)
        model.roi_heads.detector = _detector(device, cfg)
        inner = model.engine.infer_gdino

        def counted(*a, _inner=inner, _fused=fused, **k):
            fused_calls.append((_fused, k.get("prompt_depth") is not None))
            return _inner(*a, **k)
        model.engine.infer_gdino = counted
        res = [model(_text_inputs(i, device, cfg), prompt_depth=prompts[i])[0]["instances"] for i in (0, 1, 0)]
        res.append(model(_text_inputs(0, device, cfg))[0]["instances"])
        outs.append(res)
    assert fused_calls == [(True, True)] * 3 + [(True, False)]
    for k, (a, b) in enumerate(zip(*outs)):
        cases.assert_instances_equal(a, b, f"call {k}")
    cases.assert_instances_equal(outs[0][0], outs[0][2], "the same input again")
    # the detector reads only the image: the same 2D boxes, lifted from other features
    assert torch.equal(outs[0][0].pred_boxes.tensor, outs[0][3].pred_boxes.tensor)
    assert not torch.equal(outs[0][0].pred_center_cam, outs[0][3].pred_center_cam)


def _one_call_args(model, inputs):
    """(native image array kept alive, token ids, spans) of RCNN3D._infer_fused for `inputs`."""
    from ovmono3d_amd.modeling.roi_heads.gdino_glue import build_caption, phrase_spans
    images = model.preprocess_image(inputs)
    caption, _ = build_caption(list(inputs[0]["category_list"]))
    ids, phrase_ids, _ = model.roi_heads.detector._tokens(caption)
    return images, ids, phrase_spans(ids, phrase_ids)


def test_ovm_infer_depth_null_prompt_and_refusals(device, depthpro):
    """ovm_infer_depth with a null depth gives ovm_infer's records bit for bit. A prompt on a CLIP-tower handle and on a handle
    without depth_fusion weights returns the error code with its message, before anything is launched, and the next prompt-free call
    on the same handle succeeds with the records of a handle that never saw the refusal."""
    from ovmono3d_amd.lib import OVM_REC_FLOATS, OvmError
    prompt = _prompts(device, depthpro)[0]
    cfg = cases.model_cfg("ROIHeads3DGDINO")
    model, _ = _model(cfg, device, seed=3)
    model.roi_heads.detector = _detector(device, cfg)
    eng, det = model.engine, model.roi_heads.detector.engine
    inputs = _text_inputs(0, device, cfg)
    images, ids, spans = _one_call_args(model, inputs)
    nq = det.cfg.num_queries
    want, n = eng.infer_gdino(images.native, det._h, ids, spans, 0.001, 0.5, nq)                       # ovm_infer
    assert n >= 1
    rec = torch.full((nq, OVM_REC_FLOATS), -1.0, dtype=torch.float32, device=device)
    n_out = C.c_int32(0)
    ids_c = (C.c_int32 * len(ids))(*[int(v) for v in ids])
    flat = [int(v) for sp in spans for v in sp]
    rc = eng._lib.ovm_infer_depth(eng._h, det._h, images.native, None, 0, 0, ids_c, len(ids), (C.c_int32 * len(flat))(*flat), len(spans), 0.001, 0.5,
                                  rec.data_ptr(), nq, C.byref(n_out), C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    assert rc == 0 and n_out.value == n
    assert torch.equal(rec[:n].view(torch.int32), want.view(torch.int32))
    with_prompt, n_p = eng.infer_gdino(images.native, det._h, ids, spans, 0.001, 0.5, nq, prompt_depth=prompt)
    assert n_p == n and not torch.equal(with_prompt, want)
    with pytest.raises(ValueError):
        eng.infer_gdino(images.native, det._h, ids, spans, 0.001, 0.5, nq, prompt_depth=torch.cat([prompt, prompt]))

    # a handle without depth_fusion weights; its prompt-free records are those of the full checkpoint (the branch is not run)
    bare, _ = _model(cfg, device, seed=3, drop=("depth_fusion",))
    bare.roi_heads.detector = model.roi_heads.detector
    with pytest.raises(OvmError, match="depth_fusion weights absent"):
        bare.engine.infer_gdino(images.native, det._h, ids, spans, 0.001, 0.5, nq, prompt_depth=prompt)
    again, n_b = bare.engine.infer_gdino(images.native, det._h, ids, spans, 0.001, 0.5, nq)
    assert n_b == n and torch.equal(again.view(torch.int32), want.view(torch.int32))

    # a CLIP-tower handle
    ccfg = build_clip_cfg("ViT-test-16", 288, "f16x3", max_batch=1, max_rois=64, roi_heads="ROIHeads3DGDINO", extra=cases.SIZE_OPTS)
    clip, _ = _model(ccfg, device, seed=3)
    clip.roi_heads.detector = _detector(device, ccfg)
    cdet = clip.roi_heads.detector.engine
    cin = _text_inputs(0, device, ccfg)
    cimages, cids, cspans = _one_call_args(clip, cin)
    first, n_c = clip.engine.infer_gdino(cimages.native, cdet._h, cids, cspans, 0.001, 0.5, nq)
    assert n_c >= 1
    with pytest.raises(OvmError, match="only defined for the DINOv2 tower"):
        clip.engine.infer_gdino(cimages.native, cdet._h, cids, cspans, 0.001, 0.5, nq, prompt_depth=prompt)
    second, n_c2 = clip.engine.infer_gdino(cimages.native, cdet._h, cids, cspans, 0.001, 0.5, nq)
    assert n_c2 == n_c and torch.equal(second.view(torch.int32), first.view(torch.int32))
    with pytest.raises(TypeError):                                  # through the model: the staged path's refusal, as before
        clip(cin, prompt_depth=prompt)


# ------------------------------------------------------------------------------------------ entry points
TINY_MODEL = ["MODEL.DINO.MODEL_NAME", "vittest14", "MODEL.FPN.SQUARE_PAD", str(cases.CANVAS), "INPUT.MIN_SIZE_TEST", str(cases.MIN_SIZE),
              "INPUT.MAX_SIZE_TEST", str(cases.MAX_SIZE), "MODEL.WEIGHTS", f"synthetic://vittest14?seed={cases.MODEL_SEED}"]
DEPTHPRO_FLAGS = ["--depth", "depthpro", "--depthpro-weights", cases.DEPTHPRO_SPEC, "--depthpro-config", cases.DEPTHPRO_CONFIG_JSON]


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_demo_depthpro_then_files_then_none(device, tmp_path):
    inp = tmp_path / "in"
    names = cases.write_images(str(inp))
    (tmp_path / "labels.json").write_text(json.dumps({n: ["chair", "table"] for n in names}))
    (tmp_path / "boxes.json").write_text(json.dumps({n: [{"bbox": [20, 20, 60, 50], "category_id": 0, "score": 0.9},
                                                         {"bbox": [70, 40, 50, 60], "category_id": 1, "score": 0.8}] for n in names}))
    base = [sys.executable, os.path.join(ROOT, "demo", "demo.py"), "--config-file", os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml"),
            "--input-folder", str(inp), "--labels-file", str(tmp_path / "labels.json"), "--boxes-file", str(tmp_path / "boxes.json"),
            "--threshold", "0.0"]
    runs = {"depthpro": DEPTHPRO_FLAGS + ["--dump-depth", str(tmp_path / "maps")], "files": ["--depth", "files", "--depth-dir", str(tmp_path / "maps")],
            "none": []}
    for key, flags in runs.items():
        _run(base + flags + TINY_MODEL + ["MODEL.AMD.VIS", "False", "OUTPUT_DIR", str(tmp_path / key)])
        if key == "depthpro":
            for n, hw in zip(names, cases.HWS):
                z = np.load(tmp_path / "maps" / (n + ".npz"))["depth"]
                assert z.dtype == np.float32 and z.shape == hw and (z > 0).all()
    for n in names:
        a, b, c = ((tmp_path / key / f"{n}_dets.json").read_bytes() for key in runs)
        assert len(json.loads(a)["detections"]) == 2
        assert a == b, n
        assert a != c, n


def test_eval_only_depthpro_equals_depth_dir(device, tmp_path):
    root = tmp_path / "datasets"
    (root / "Omni3D").mkdir(parents=True)
    names = cases.write_images(str(root / "imgs"))
    images = [{"id": 100 + i, "file_path": f"imgs/{n}.png", "width": cases.HWS[i][1], "height": cases.HWS[i][0], "dataset_id": 0,
               "K": cases.intrinsics(i)} for i, n in enumerate(names)]
    c3 = [[x, y, z] for z in (4.5, 5.5) for (x, y) in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5))]
    ann = {"valid3D": True, "dimensions": [1.0, 1.0, 1.0], "lidar_pts": -1, "segmentation_pts": -1, "depth_error": -1, "truncation": 0.0,
           "visibility": 1.0, "bbox2D_trunc": [-1, -1, -1, -1], "bbox2D_tight": [-1, -1, -1, -1], "R_cam": np.eye(3).tolist(),
           "bbox3D_cam": c3, "center_cam": [0, 0, 5.0], "behind_camera": False, "id": 1, "image_id": 100, "category_id": 18,
           "category_name": "chair", "bbox2D_proj": [20, 20, 80, 70]}
    cats = [{"id": i, "name": n} for i, n in zip((11, 14, 15, 16, 17, 18, 19, 20, 21),
                                                 ("bicycle", "books", "bottle", "camera", "cereal box", "chair", "cup", "laptop", "shoes"))]
    (root / "Omni3D" / "Objectron_test.json").write_text(json.dumps({"info": {"name": "Objectron"}, "images": images, "annotations": [ann],
                                                                     "categories": cats}))
    base = [sys.executable, os.path.join(ROOT, "tools", "train_net.py"), "--eval-only", "--config-file",
            os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml"), "--datasets-root", str(root / "Omni3D"), "--image-root", str(root)]
    opts = TINY_MODEL + ["DATASETS.TEST_BASE", "('Objectron_test',)", "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.0"]
    runs = {"depthpro": DEPTHPRO_FLAGS + ["--depthpro-focal", "K", "--dump-depth", str(tmp_path / "maps" / "test")],
            "files": ["--depth-dir", str(tmp_path / "maps")]}
    res = {}
    for key, flags in runs.items():
        _run(base + flags + opts + ["OUTPUT_DIR", str(tmp_path / key)])
        res[key] = (tmp_path / key / "inference" / "iter_final" / "Objectron_test" / "omni_instances_results.json").read_bytes()
        if key == "depthpro":
            assert sorted(os.listdir(tmp_path / "maps" / "test")) == [n + ".npz" for n in names]
    assert len(json.loads(res["depthpro"])) > 0
    assert res["depthpro"] == res["files"]
