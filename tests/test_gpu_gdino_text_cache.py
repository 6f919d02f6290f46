"""The detector's caption cache (ovm_tune_set gdino_text_cache, default 16): what depends on the caption and the weights alone - BERT, the
text projection, encoder layer 0's text norm and text projection - is computed once per (token ids, position ids, tune generation),
outside the per-image graph, into an entry that the handle keeps and every plan of that caption co-owns. Same kernels on the same
operands in the same order as inside a forward, so logits and boxes must equal, bit for bit, those of a fresh engine built with
gdino_text_cache = 0 ("the uncached engine" below), which encodes inside every forward."""
from contextlib import contextmanager

import pytest
import torch

from test_gpu_gdino_engine import SMALL, _engine, _hf_small_pair

pytestmark = pytest.mark.gpu

CAP_A = [101, 500, 1012, 600, 601, 1012, 700, 1012, 102]           # 9 tokens
CAP_B = [101, 510, 1012, 610, 611, 1012, 710, 1012, 102]           # same length and delimiters, other words
CAP_C = [101, 520, 521, 1012, 102]                                 # 5 tokens
HW1, HW2 = (64, 80), (96, 64)
BERT_LAYERS = 2                                                    # test_gpu_gdino._small_hf_gdino's text model
ENC_OPS = 1 + 7 * BERT_LAYERS + 1                                  # embedding, 7 ops per BERT layer, the text projection


@contextmanager
def _knobs(restore, **kw):
    """ovm_tune_set for the body; `restore`: the values put back afterwards (every call advances the tune generation)"""
    from ovmono3d_amd import lib
    L = lib.load()
    try:
        for k, v in kw.items():
            assert L.ovm_tune_set(k.encode(), v) == 0, k
        yield
    finally:
        for k, v in restore.items():
            L.ovm_tune_set(k.encode(), v)


def _sd():
    return _hf_small_pair()[0].state_dict()


def _img(device, hw, seed):
    return torch.randint(0, 256, (3,) + hw, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(device)


def _uncached(device, calls, sd=None, cfg=SMALL, taps=(), **tune):
    """a fresh engine under gdino_text_cache = 0 (and `tune`): (logits, boxes) of every (image, ids, position ids) call, the launch
    count of the last one, and the named taps after it"""
    restore = dict(gdino_text_cache=16, **{k: tune[k][1] for k in tune})
    with _knobs(restore, gdino_text_cache=0, **{k: tune[k][0] for k in tune}):
        eng = _engine(device, sd if sd is not None else _sd(), cfg, use_graphs=False)
        outs = [tuple(t.clone() for t in eng.forward(im, ids, pids)) for im, ids, pids in calls]
        assert eng.debug_scalar("text_entries") == 0 and eng.debug_scalar("text_launches") == 0
        got = {name: eng.debug(name, shape).clone() for name, shape in taps}
        return outs, eng.launches(), got


def _same(got, want, what):
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what


def test_eager_call_and_replays_equal_the_uncached_engine(device):
    a, b = _img(device, HW1, 1), _img(device, HW1, 2)
    ref, _, _ = _uncached(device, [(a, CAP_A, None), (b, CAP_A, None)])
    eng = _engine(device, _sd(), SMALL, use_graphs=True)
    _same(eng.forward(a, CAP_A), ref[0], "first call (eager, encodes the caption)")
    assert eng.debug_scalar("text_launches") == ENC_OPS + 2 and eng.debug_scalar("text_entries") == 1
    _same(eng.forward(a, CAP_A), ref[0], "second call (replay)")
    assert eng.debug_scalar("text_launches") == 0
    _same(eng.forward(b, CAP_A), ref[1], "third call (replay, another image)")


def test_second_shape_of_a_caption_runs_no_text_encoder(device):
    a, b = _img(device, HW1, 3), _img(device, HW2, 4)
    ref, _, _ = _uncached(device, [(a, CAP_A, None), (b, CAP_A, None)])
    for graphs in (False, True):
        eng = _engine(device, _sd(), SMALL, use_graphs=graphs)
        _same(eng.forward(a, CAP_A), ref[0], "first shape")
        assert eng.debug_scalar("text_launches") > 0
        _same(eng.forward(b, CAP_A), ref[1], "second shape, first forward")
        assert eng.debug_scalar("text_launches") == 0 and eng.debug_scalar("text_entries") == 1 and eng.debug_scalar("plans") == 2
        _same(eng.forward(b, CAP_A), ref[1], "second shape again")
        _same(eng.forward(a, CAP_A), ref[0], "first shape again")


PIDS_A = [0, 0, 1, 0, 1, 2, 0, 1, 0]                                # upstream numbering of CAP_A
NEAR = {
    "same-length-other-ids": ((CAP_A, None), (CAP_B, None)),
    "same-ids-other-position-ids": ((CAP_A, PIDS_A), (CAP_A, [0, 1, 2, 3, 4, 5, 6, 7, 8])),
    "explicit-vs-default-position-ids": ((CAP_A, None), (CAP_A, [0, 1, 2, 3, 4, 5, 6, 7, 8])),
    "strict-prefix": ((CAP_A, None), (CAP_A[:6], None)),
}


@pytest.mark.parametrize("case", sorted(NEAR))
def test_near_miss_keys_get_their_own_entry(device, case):
    """one engine, one shape, the first caption, the near miss, the first again: each equals its own uncached run"""
    first, second = NEAR[case]
    im = _img(device, HW1, 5)
    calls = [(im,) + first, (im,) + second]
    ref, _, _ = _uncached(device, calls)
    eng = _engine(device, _sd(), SMALL, use_graphs=True)
    for rnd in range(2):
        for i, (_, ids, pids) in enumerate(calls):
            _same(eng.forward(im, ids, pids), ref[i], (case, rnd, i))
            assert eng.debug_scalar("text_launches") == (ENC_OPS + 2 if rnd == 0 else 0), (case, rnd, i)
    assert eng.debug_scalar("text_entries") == 2


def test_tune_set_retires_the_entries_made_before_it(device):
    """glin_max_ksplit changes how the small GEMMs split K, i.e. their summation order: after the call the caption is encoded anew, for
    a new shape and for an eager pass over the old plan alike, and both equal a fresh uncached engine under that knob"""
    a, b = _img(device, HW1, 6), _img(device, HW2, 7)
    ref, _, _ = _uncached(device, [(a, CAP_A, None), (b, CAP_A, None)], glin_max_ksplit=(1, 16))
    eng = _engine(device, _sd(), SMALL, use_graphs=False)
    eng.forward(a, CAP_A)
    assert eng.debug_scalar("text_entries") == 1
    with _knobs(dict(glin_max_ksplit=16), glin_max_ksplit=1):
        _same(eng.forward(b, CAP_A), ref[1], "new shape after the knob changed")
        assert eng.debug_scalar("text_launches") == ENC_OPS + 2 and eng.debug_scalar("text_entries") == 2
        _same(eng.forward(a, CAP_A), ref[0], "eager pass over the old plan after the knob changed")
        assert eng.debug_scalar("text_launches") == 0 and eng.debug_scalar("text_entries") == 2      # the entry made for the new shape


def test_eviction_never_frees_what_a_live_graph_reads(device):
    """capacity 2; captions A, B, C, then A on its old plan (whose entry has left the handle's list) and on a new shape"""
    ims = [_img(device, HW1, 8 + i) for i in range(4)]
    new = _img(device, HW2, 12)
    ref, _, _ = _uncached(device, [(ims[0], CAP_A, None), (ims[1], CAP_B, None), (ims[2], CAP_C, None), (ims[3], CAP_A, None),
                                    (new, CAP_A, None), (ims[1], CAP_A, None)])
    with _knobs(dict(gdino_text_cache=16), gdino_text_cache=2):
        eng = _engine(device, _sd(), SMALL, use_graphs=True)
        _same(eng.forward(ims[0], CAP_A), ref[0], "A")
        _same(eng.forward(ims[1], CAP_B), ref[1], "B")
        assert eng.debug_scalar("text_entries") == 2
        _same(eng.forward(ims[2], CAP_C), ref[2], "C")
        assert eng.debug_scalar("text_entries") == 2 and eng.debug_scalar("plans") == 3
        _same(eng.forward(ims[3], CAP_A), ref[3], "A's old graph after its entry left the list")
        assert eng.debug_scalar("text_launches") == 0
        _same(eng.forward(new, CAP_A), ref[4], "A on a new shape: encoded again")
        assert eng.debug_scalar("text_launches") == ENC_OPS + 2 and eng.debug_scalar("text_entries") == 2
        _same(eng.forward(ims[1], CAP_A), ref[5], "A's old graph beside the new entry")
        _same(eng.forward(ims[1], CAP_B), ref[1], "B's graph")
        _same(eng.forward(ims[2], CAP_C), ref[2], "C's graph")


def test_entry_made_on_one_stream_serves_another_without_a_host_sync(device):
    a, b = _img(device, HW1, 13), _img(device, HW2, 14)
    ref, _, _ = _uncached(device, [(a, CAP_A, None), (b, CAP_A, None)])
    eng = _engine(device, _sd(), SMALL, use_graphs=True)
    sx, sy = torch.cuda.Stream(device), torch.cuda.Stream(device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(sx):
        out_x = eng.forward(a, CAP_A)                              # the miss: encodes on stream X
    with torch.cuda.stream(sy):
        out_y = eng.forward(b, CAP_A)                              # the same caption, a new shape, stream Y
        assert eng.debug_scalar("text_launches") == 0
    torch.cuda.synchronize(device)
    _same(out_x, ref[0], "stream X")
    _same(out_y, ref[1], "stream Y")


def test_taps_point_into_the_entry(device):
    a = _img(device, HW1, 15)
    T = len(CAP_A)
    taps = (("bert_out", (T, 64)), ("text_features", (T, 64)))
    _, _, want = _uncached(device, [(a, CAP_A, None)], taps=taps)
    eng = _engine(device, _sd(), SMALL, use_graphs=True)
    for _ in range(2):
        eng.forward(a, CAP_A)                                      # eager, then a replay
    for name, shape in taps:
        assert torch.equal(eng.debug(name, shape), want[name]), name


def test_launches_is_the_per_image_count(device):
    a = _img(device, HW1, 16)
    _, off, _ = _uncached(device, [(a, CAP_A, None)])
    for graphs in (False, True):
        eng = _engine(device, _sd(), SMALL, use_graphs=graphs)
        counts = []
        for _ in range(3):
            eng.forward(a, CAP_A)
            counts.append(eng.launches())
        print(f"launches per forward: {off} with the encoder inside, {counts[0]} with the caption entry")
        assert counts[0] == off - ENC_OPS - 2                      # the encoder's ops, layer 0's text norm and text projection
        assert counts[1] == counts[0] and counts[2] == counts[0]


def test_full_size_bench_caption_is_bit_identical(device):
    """Swin-B / BERT-base / 900 queries, synthetic weights, 532 x 532, the six categories of bench.py"""
    from ovmono3d_amd.gdino.detector import HashTokenizer
    from ovmono3d_amd.modeling.roi_heads.gdino_glue import build_caption
    from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict
    sd = synth_gdino_state_dict(3)
    ids = HashTokenizer().encode(build_caption(["chair", "dining table", "sofa", "potted plant", "television", "bookcase"])[0])
    im = _img(device, (532, 532), 17)
    ref, off, _ = _uncached(device, [(im, ids, None)], sd=sd, cfg={})
    eng = _engine(device, sd, {}, use_graphs=True)
    _same(eng.forward(im, ids), ref[0], "eager")
    assert eng.debug_scalar("text_launches") == 1 + 7 * 12 + 1 + 2
    _same(eng.forward(im, ids), ref[0], "replay")
    assert eng.launches() == off - (1 + 7 * 12 + 1) - 2
