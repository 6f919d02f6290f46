"""The depth prompt from Depth Pro, host side (ovmono3d_amd/data/depth_prompt.py): the flags of demo/demo.py and tools/train_net.py
and their refusals (argparse errors before any device call), the ``synthetic://depthpro`` spec, the data mapper's two depth routes on
the host path, and the condition of the GPU tests: on the oracle alone, the depth of the fp64 Hugging Face Depth Pro moves the tiny
model's detections by at least 10 x the parity tolerance, so a dropped prompt cannot pass test_gpu_depth_prompt.py's parity check."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from common import ROOT, oracle_params
import depth_prompt_cases as cases

CONFIG = os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml")
DEMO = [sys.executable, os.path.join(ROOT, "demo", "demo.py"), "--config-file", CONFIG, "--input-folder", "nowhere", "--labels-file", "nothing.json"]
TRAIN = [sys.executable, os.path.join(ROOT, "tools", "train_net.py"), "--eval-only", "--config-file", CONFIG]
DP = ["--depth", "depthpro", "--depthpro-weights", cases.DEPTHPRO_SPEC]
CLIP = ["--config-file", os.path.join(ROOT, "configs", "OVMono3D_clip_SFP.yaml")]

REFUSALS = [
    # (flags, configuration overrides, what stderr must name)
    (["--depth", "depthpro"], [], "--depthpro-weights"),
    (DP + ["--depth-dir", "maps"], [], "--depth-dir"),
    (DP + CLIP, [], "MODEL.BACKBONE.NAME"),
    (DP, ["MODEL.DINO.USE_DEPTH_FUSION", "False"], "MODEL.DINO.USE_DEPTH_FUSION"),
    (DP, ["MODEL.DINO.MODEL_NAME", "vitb14_reg"], "MODEL.DINO.MODEL_NAME"),
]


@pytest.mark.parametrize("entry", ["demo", "train_net"])
@pytest.mark.parametrize("flags,opts,named", REFUSALS)
def test_entry_points_refuse_before_any_device_call(entry, flags, opts, named):
    """Exit status 2 (an argparse error) naming the flag or the setting; this machine has no device, so anything later would fail
    otherwise (and with another status)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run((DEMO if entry == "demo" else TRAIN) + flags + opts, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr[-1500:])
    assert "error:" in r.stderr and named in r.stderr.split("error:")[-1], r.stderr[-1500:]


def test_demo_files_route_needs_a_folder():
    r = subprocess.run(DEMO + ["--depth", "files"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--depth-dir" in r.stderr.split("error:")[-1], r.stderr[-1500:]


def test_default_flags_are_todays_behaviour():
    """No new flag: demo.py has no depth, train_net.py reads files from an optional --depth-dir."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_net_for_depth_prompt", os.path.join(ROOT, "tools", "train_net.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.default_argument_parser().parse_args(["--eval-only"])
    assert a.depth == "files" and a.depth_dir is None and a.depthpro_weights is None and a.dump_depth is None and a.depthpro_focal == "estimate"
    a = mod.default_argument_parser().parse_args(["--eval-only", "--depth-dir", "maps"])
    assert a.depth == "files" and a.depth_dir == "maps"


def test_synthetic_depthpro_spec():
    from ovmono3d_amd.data.depth_prompt import synthetic_depthpro_spec
    assert synthetic_depthpro_spec("synthetic://depthpro?seed=11&crop=128") == (11, 128)
    assert synthetic_depthpro_spec("synthetic://depthpro?crop=384") == (0, 384)
    assert synthetic_depthpro_spec("synthetic://depthpro") == (0, None)
    assert synthetic_depthpro_spec(cases.DEPTHPRO_SPEC) == (cases.TINY["seed"], cases.TINY["config"]["crop"])
    for bad in ("synthetic://gdino?seed=1", "synthetic://depthpro?seed=x", "synthetic://depthpro?sed=1", "synthetic://depthpro?seed=1&seed=2",
                "synthetic://depthpro?seed", "synthetic://depthpro/v2?seed=1", "synthetic://depthpro?crop=0", "file://depthpro?seed=1"):
        with pytest.raises(ValueError):
            synthetic_depthpro_spec(bad)


def test_geo_tool_keeps_its_depth_file_helpers(tmp_path):
    """dump_depth / load_depth live in the package; tools/ovmono3d_geo.py reads with that load_depth (Depth Pro's maps are dumped by
    DepthProPrompt, with that dump_depth) and a dumped map is found again, under <dir> and under <dir>/test, with GEO's shape check only
    when a size is given."""
    import importlib.util
    from ovmono3d_amd.data import depth_prompt
    spec = importlib.util.spec_from_file_location("geo_for_depth_prompt", os.path.join(ROOT, "tools", "ovmono3d_geo.py"))
    geo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(geo)
    assert geo.load_depth is depth_prompt.load_depth
    ramp = torch.arange(12, dtype=torch.float32).reshape(3, 4) / 7
    depth_prompt.dump_depth(str(tmp_path / "test"), "some/where/a.b.jpg", ramp)
    assert (tmp_path / "test" / "a.b.npz").exists()
    got = geo.load_depth(str(tmp_path), "other/a.b.png", 3, 4)
    assert got.dtype == np.float32 and np.array_equal(got, ramp.numpy())
    assert np.array_equal(depth_prompt.load_depth(str(tmp_path / "test"), "a.b.png"), ramp.numpy())
    with pytest.raises(SystemExit, match="resolution"):
        geo.load_depth(str(tmp_path), "a.b.png", 4, 3)
    with pytest.raises(SystemExit, match="c.png"):
        depth_prompt.load_depth(str(tmp_path), "c.png")


class _RampSource:
    """A fixed fp32 ramp of another size than the image's: 45 x 70."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def ramp():
        return (0.5 + torch.arange(45 * 70, dtype=torch.float32).reshape(45, 70) / 400.0) ** 1.5

    def __call__(self, image, image_format, K, file_name=None):
        self.calls.append((tuple(image.shape), image_format, float(K[0][0]), file_name))
        return self.ramp()


def test_mapper_source_route_equals_file_route_on_the_host(tmp_path):
    from ovmono3d_amd.data import DatasetMapper3D
    cfg = cases.model_cfg(gpu_resize=False)
    names = cases.write_images(str(tmp_path / "imgs"))
    dicts = cases.dataset_dicts(str(tmp_path / "imgs"), names)
    (tmp_path / "maps" / "test").mkdir(parents=True)
    for n in names:
        np.savez(tmp_path / "maps" / "test" / (n + ".npz"), depth=_RampSource.ramp().numpy())
    src = _RampSource()
    inline, files = DatasetMapper3D(cfg, False, depth_source=src), DatasetMapper3D(cfg, False, str(tmp_path / "maps"))
    for i, d in enumerate(dicts):
        a, b = inline(d), files(d)
        h, w = cases.HWS[i]
        nh, nw = (140, 187) if h < w else (187, 140)
        assert tuple(a["image"].shape) == (3, nh, nw) and tuple(a["depth"].shape) == (1, nh, nw) and a["depth"].dtype == torch.float32
        assert torch.equal(a["depth"], b["depth"]) and torch.equal(a["image"], b["image"])
        assert src.calls[i] == ((h, w, 3), cfg.INPUT.FORMAT, 300.0, d["file_name"])
        # and it is the reference's two resizes (dataset_mapper.py:45-52,70-72)
        want = _RampSource.ramp()[None, None]
        for size in ((h, w), (nh, nw)):
            want = torch.nn.functional.interpolate(want, size=size, mode="bilinear", align_corners=False)
        assert torch.equal(a["depth"], want[0])
    # nothing reads a depth: the source is not called
    for extra in (["MODEL.DINO.USE_DEPTH_FUSION", False], ["MODEL.DINO.MODEL_NAME", "vittest14_reg"]):
        quiet = _RampSource()
        rec = DatasetMapper3D(cases.model_cfg(gpu_resize=False, extra=extra), False, depth_source=quiet)(dicts[0])
        assert "depth" not in rec and quiet.calls == []


def test_mapper_without_source_still_gives_zeros_for_an_unreadable_file(tmp_path):
    from ovmono3d_amd.data import DatasetMapper3D
    cfg = cases.model_cfg(gpu_resize=False)
    names = cases.write_images(str(tmp_path / "imgs"))
    dicts = cases.dataset_dicts(str(tmp_path / "imgs"), names)
    (tmp_path / "maps" / "test").mkdir(parents=True)
    (tmp_path / "maps" / "test" / (names[1] + ".npz")).write_bytes(b"not a zip file")
    mapper = DatasetMapper3D(cfg, False, str(tmp_path / "maps"), depth_source=None)
    for d, shape in zip(dicts, ((1, 140, 187), (1, 187, 140))):           # a missing file, a broken one
        rec = mapper(d)
        assert tuple(rec["depth"].shape) == shape and rec["depth"].dtype == torch.float32 and not rec["depth"].any()
    assert "depth" not in DatasetMapper3D(cfg, False)(dicts[0])


def test_oracle_condition_the_depth_prompt_moves_the_detections():
    """The condition of test_gpu_depth_prompt.py's parity check, on the oracle alone: the depth of the fp64 Hugging Face run of the
    TINY Depth Pro, through prepare_prompt_depth, moves at least one float field of the tiny model's detections on given boxes by
    10 x the parity tolerance of tests/test_gpu_model.py's depth-prompt test (1e-3, scale-relative). A failure means the synthetic
    depth_fusion weights or the image need changing, not the factor."""
    from depthpro_oracle import TINY, reference_pair
    from oracle.pipeline import inference
    from ovmono3d_amd.data import ResizeShortestEdge
    from ovmono3d_amd.data.depth_prompt import prepare_prompt_depth
    from ovmono3d_amd.util.synth_weights import synth_state_dict
    cfg = cases.model_cfg(gpu_resize=False)
    sd = synth_state_dict("vittest14", num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, seed=cases.MODEL_SEED)
    r64 = reference_pair(TINY)[0]
    depth = prepare_prompt_depth(r64["depth_est"].float().numpy(), cases.HWS[0], ResizeShortestEdge(cases.MIN_SIZE, cases.MAX_SIZE))
    assert tuple(depth.shape) == (140, 187)
    inputs = [cases.model_input(0, cfg.INPUT.FORMAT)]
    plain = inference(sd, inputs, oracle_params(cfg))[0]
    prompted = inference(sd, inputs, oracle_params(cfg), prompt_depth=depth[None, None])[0]
    assert len(plain["scores"]) == len(prompted["scores"]) == 6
    move = cases.max_field_move(prompted, plain)
    print(f"largest scale-relative move of a float field under the depth prompt: {move:.3e} (needed: {cases.MARGIN:.1e})")
    assert move >= cases.MARGIN
