"""CPU: the two OVMono3D-GEO front ends (tools/ovmono3d_geo.py, demo/demo_geo.py) and demo/demo.py keep their command lines - every
flag's dest, default, choices, nargs, required and type as recorded in tests/golden/geo_cli_flags.json before the shared declarations
(``add_depth_arguments``, ``add_mask_arguments``, ``add_ply_arguments``) replaced the scripts' own -, refuse what cannot work with exit
status 2, borrow nothing from another script, and ``geo.sources.planes_on_device`` makes one tensor of planes from either side."""
import ast
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from common import ROOT

SCRIPTS = ("tools/ovmono3d_geo.py", "demo/demo_geo.py", "demo/demo.py")


def _script(rel):
    spec = importlib.util.spec_from_file_location("frontend_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flag_table(parser):
    table = {}
    for a in parser._actions:
        table[",".join(a.option_strings) or a.dest] = [a.dest, a.default, None if a.choices is None else list(a.choices), a.nargs, a.required,
                                                       None if a.type is None else a.type.__name__]
    return json.loads(json.dumps(table))


@pytest.mark.parametrize("rel", SCRIPTS)
def test_flag_surface_is_the_recorded_one(rel):
    with open(os.path.join(ROOT, "tests", "golden", "geo_cli_flags.json")) as f:
        want = json.load(f)[rel]
    assert _flag_table(_script(rel).argument_parser()) == want


TOOL = ["--oracle2d", "o", "--dataset", "d", "--output", "out.pth"]
DEMO = ["--input-folder", "x", "--labels-file", "l"]
FILES = ["--depth", "files", "--depth-dir", "d"]
REFUSALS = [
    ("tool", TOOL + ["--mask", "box", "--depth", "files"], "--depth-dir"),
    ("demo", DEMO + ["--mask", "box", "--depth", "files"], "--depth-dir"),
    ("tool", TOOL + ["--mask", "box", "--depth", "depthpro", "--depthpro-weights", "w", "--depth-dir", "d"], "would not be read"),
    ("demo", DEMO + ["--mask", "box", "--depth", "depthpro", "--depthpro-weights", "w", "--depth-dir", "d"], "would not be read"),
    ("tool", TOOL + FILES + ["--mask", "box", "--dump-depth", "out"], "--dump-depth"),
    ("demo", DEMO + FILES + ["--mask", "box", "--dump-depth", "out"], "--dump-depth"),
    ("tool", TOOL + FILES + ["--mask", "sam", "--sam-weights", "w", "--sam-refine", "-1"], "--sam-refine"),
    ("demo", DEMO + FILES + ["--mask", "sam", "--sam-weights", "w", "--sam-refine", "-1"], "--sam-refine"),
    ("tool", TOOL + FILES + ["--mask", "box", "--sam-refine", "1"], "--sam-refine"),
    ("demo", DEMO + FILES + ["--mask", "box", "--sam-refine", "1"], "--sam-refine"),
    ("tool", TOOL + FILES + ["--mask", "box", "--min-mask-region-area", "-1"], "--min-mask-region-area"),
    ("demo", DEMO + FILES + ["--mask", "box", "--min-mask-region-area", "-1"], "--min-mask-region-area"),
    ("demo", ["--input-folder", "x"] + FILES + ["--everything", "--sam-weights", "w", "--points-file", "p.json"], "neither --points-file nor --boxes-file"),
    ("demo", ["--input-folder", "x"] + FILES + ["--everything", "--mask", "box"], "needs --mask sam"),
    ("demo", ["--input-folder", "x"] + FILES + ["--everything", "--sam-weights", "w", "--points-per-side", "37"], "--points-per-side"),
    ("demo", ["--input-folder", "x"] + FILES + ["--sam-weights", "w", "--points-file", "p.json", "--boxes-file", "b.json"], "give one"),
    ("demo", ["--input-folder", "x"] + FILES + ["--mask", "box"], "--labels-file"),
    ("demo", DEMO + FILES + ["--mask", "sam"], "--sam-weights"),
]


@pytest.mark.parametrize("which,argv,msg", REFUSALS)
def test_refusals_exit_with_status_2(which, argv, msg, capsys):
    mod = _script("tools/ovmono3d_geo.py" if which == "tool" else "demo/demo_geo.py")
    parser = mod.argument_parser()
    args = parser.parse_args(argv)
    with pytest.raises(SystemExit) as e:
        (mod.check_args if which == "tool" else mod.check_arguments)(args, parser)
    assert e.value.code == 2 and msg in capsys.readouterr().err


@pytest.mark.parametrize("rel", SCRIPTS[:2])
def test_front_ends_borrow_nothing_from_another_script(rel):
    with open(os.path.join(ROOT, rel)) as f:
        tree = ast.parse(f.read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            imported.add((node.module or "").split(".")[0])
    assert "ovmono3d_amd" in imported and not imported & {"demo", "make_oracle2d", "ovmono3d_geo"}


def test_planes_on_device_takes_planes_from_either_side():
    from ovmono3d_amd.geo.sources import planes_on_device
    rng = np.random.RandomState(5)
    want = (rng.rand(4, 6, 10) > 0.5).astype(np.uint8)
    cpu = torch.device("cpu")
    strided = np.asfortranarray(want[2])                                     # a plane that is not C-contiguous
    wide = np.zeros((6, 20), np.uint8)
    wide[:, ::2] = want[3]
    assert not strided.flags["C_CONTIGUOUS"] and not wide[:, ::2].flags["C_CONTIGUOUS"]
    for planes in ([p for p in want], [torch.from_numpy(p.copy()) for p in want], torch.from_numpy(want.copy()),
                   [want[0], torch.from_numpy(want[1].copy()), strided, wide[:, ::2]]):
        got = planes_on_device(planes, cpu)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 6, 10) and got.device == cpu
        assert np.array_equal(got.numpy(), want)
