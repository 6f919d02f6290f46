"""GPU: the device entropy route (ovmono3d_amd/csrc/jpeg_dec.hip) against the host decoder's planes, bit for bit, on the files of
tests/jpeg_entropy_cases.py (whose conditions tests/test_jpeg_entropy_cpu.py asserts, and which pass the CPU emulation there)."""
import io

import numpy as np
import pytest
import torch

import jpeg_entropy_cases as K
from test_jpeg import _jpeg, _pil, _scene
from ovmono3d_amd.data import gpu_jpeg

pytestmark = pytest.mark.gpu

NAMES = sorted(K.well_formed())


@pytest.mark.parametrize("name", NAMES)
def test_device_planes_equal_host_decoder(device, name):
    data = K.well_formed()[name]
    want, winfo = K.host_planes(name)
    got, info, status, rounds = gpu_jpeg.entropy_decode_device(data, device)
    assert status == 0, f"declined a well-formed file: status {status}"
    assert got.dtype == torch.int16 and got.is_cuda and tuple(got.shape) == tuple(want.shape)
    bad = (got.cpu() != want).any(1).nonzero().flatten()
    assert len(bad) == 0, f"{len(bad)} of {len(want)} blocks differ, first {bad[:4].tolist()}"
    assert rounds == K.emulated(name)[3], "the kernels' round schedule differs from the emulation's"
    assert np.array_equal(gpu_jpeg.decode_jpeg(data, device, entropy="device").cpu().numpy(), _pil(data))


def test_full_hd_picture_repeat_and_stream_offset(device):
    """Launch shapes of a large file (many workgroups, several scan tiles); two calls give equal bytes; the stream may start at
    any byte of its buffer."""
    data = _jpeg(_scene(1080, 1920, 9), quality=90, subsampling=2)
    want, _ = gpu_jpeg.entropy_decode(data)
    a, info, status, rounds = gpu_jpeg.entropy_decode_device(data, device)
    assert status == 0 and torch.equal(a.cpu(), want)
    b, _, status_b, rounds_b = gpu_jpeg.entropy_decode_device(data, device)
    assert (status_b, rounds_b) == (0, rounds) and torch.equal(a, b)
    assert np.array_equal(gpu_jpeg.decode_jpeg(data, device, entropy="device").cpu().numpy(), _pil(data))
    small = K.well_formed()["420_q75"]
    ref, _ = K.host_planes("420_q75")
    for off in (1, 2, 3, 7, 13):
        got, _, status, _ = gpu_jpeg.entropy_decode_device(small, device, stream_offset=off)
        assert status == 0 and torch.equal(got.cpu(), ref), off


def _device_or_none(data, device, max_rounds=None):
    try:
        coef, info, status, rounds = gpu_jpeg.entropy_decode_device(data, device, max_rounds=max_rounds)
    except gpu_jpeg.EntropyDeclined:
        return None
    return coef if status == 0 else None


@pytest.mark.parametrize("kind", sorted(K.small_files()))
def test_listed_damage_is_declined_or_equal_to_the_host(device, kind):
    """The fixed list of 32 mutations per file (K.fixed_mutations), which the CPU emulation and the sanitizer program
    (scratch/fuzz_jpeg_dec.cpp --list) have passed: status non-zero, or planes equal to the host decoder's."""
    data = K.small_files()[kind]
    outcomes = [K.judge_damaged(d, _device_or_none(d, device)) for d in K.fixed_mutations(data)]
    assert len(outcomes) == 32 and not all(outcomes)
    # and the device agrees with the emulation on which ones it declines
    for d, ok in zip(K.fixed_mutations(data), outcomes):
        try:
            status = gpu_jpeg.entropy_decode_emulated(d)[2]
        except gpu_jpeg.EntropyDeclined:
            status = -1
        assert ok == (status == 0)


def test_round_cap_falls_back_to_the_host(device):
    data = K.well_formed()["scene_300x400_q95"]
    coef, info, status, rounds = gpu_jpeg.entropy_decode_device(data, device, max_rounds=1)
    assert status & 4 and rounds == gpu_jpeg.entropy_decode_emulated(data, max_rounds=1)[3]
    assert np.array_equal(gpu_jpeg.decode_jpeg(data, device, entropy="device", max_rounds=1).cpu().numpy(), _pil(data))
    prog = _jpeg(_scene(40, 56, 1), quality=80, progressive=True)      # declined by the plan: the host route, same pixels
    assert np.array_equal(gpu_jpeg.decode_jpeg(prog, device, entropy="device").cpu().numpy(), _pil(prog))
    with pytest.raises(ValueError):
        gpu_jpeg.decode_jpeg(data, device, entropy="gpu")


def test_config_key_reaches_the_reader(device, tmp_path, monkeypatch):
    """MODEL.AMD.GPU_JPEG_ENTROPY (default off) -> DatasetMapper3D -> read_image_device(entropy="device")."""
    from ovmono3d_amd.config import get_cfg, get_cfg_defaults
    from ovmono3d_amd.data import feeding
    path = str(tmp_path / "a.jpg")
    data = K.well_formed()["420_restart_rows"]
    open(path, "wb").write(data)
    seen = []
    real = gpu_jpeg.entropy_decode_device
    monkeypatch.setattr(gpu_jpeg, "entropy_decode_device", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    cfg = get_cfg_defaults(get_cfg())
    assert cfg.MODEL.AMD.GPU_JPEG_ENTROPY is False
    cfg.MODEL.DEVICE = "cuda"
    for on in (False, True):
        cfg.MODEL.AMD.GPU_JPEG_ENTROPY = on
        mapper = feeding.DatasetMapper3D(cfg, is_train=False)
        assert mapper.gpu_jpeg and mapper.jpeg_entropy == ("device" if on else "host")
        before = len(seen)
        img = gpu_jpeg.read_image_device(path, mapper.image_format, device, entropy=mapper.jpeg_entropy)
        assert (len(seen) - before) == (1 if on else 0)
        assert np.array_equal(img.cpu().numpy(), feeding.read_image(path, mapper.image_format))
