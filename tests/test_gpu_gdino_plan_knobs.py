"""The detector's tune knobs are a property of the plan: a plan keeps the values it was built under for every later pass over it (the
arena was sized for that allocation and launch sequence), and only plans built afterwards pick a new value up."""
import pytest
import torch

from test_gpu_gdino import _small_hf_gdino
from test_gpu_gdino_engine import SMALL, _engine

pytestmark = pytest.mark.gpu


def test_knob_set_between_forwards_reaches_new_plans_only(device):
    """ovm_tune_set gdino_dec_chain = 0 after a plan's first forward (use_graphs = 0, so every call walks forward_impl again): the
    second call on that plan repeats the first bit for bit with the same launch count; a new shape on the same engine is a new
    plan and runs the launch-per-op decoder - more launches than a fresh engine's row-chain plan of that shape by at least the
    bound of test_decoder_row_chain_matches_launch_per_op_decoder, 15 per decoder layer."""
    from ovmono3d_amd import lib
    L = lib.load()
    hf, _ = _small_hf_gdino()
    sd = hf.state_dict()
    g = torch.Generator().manual_seed(21)
    ids = [101, 500, 1012, 600, 601, 1012, 102]
    small = torch.randint(0, 256, (3, 96, 132), dtype=torch.uint8, generator=g).to(device)
    large = torch.randint(0, 256, (3, 160, 200), dtype=torch.uint8, generator=g).to(device)
    eng = _engine(device, sd, SMALL, use_graphs=False)
    logits, boxes = (t.clone() for t in eng.forward(small, ids))
    launches = eng.launches()
    try:
        assert L.ovm_tune_set(b"gdino_dec_chain", 0) == 0
        logits2, boxes2 = eng.forward(small, ids)
        print(f"same plan after the knob changed: {launches} -> {eng.launches()} launches")
        assert eng.launches() == launches
        assert torch.equal(logits2, logits) and torch.equal(boxes2, boxes)
        eng.forward(large, ids)
        per_op = eng.launches()
    finally:
        L.ovm_tune_set(b"gdino_dec_chain", 1)
    fresh = _engine(device, sd, SMALL, use_graphs=False)
    fresh.forward(large, ids)
    print(f"160 x 200: new plan under the knob {per_op} launches, fresh engine {fresh.launches()}")
    assert per_op >= fresh.launches() + 15 * SMALL["dec_layers"]
