"""GPU, two devices: the launch forms whose dynamic LDS the device has to grant run on a second device of the process as on the first.

The grants (hipFuncAttributeMaxDynamicSharedMemorySize) are kept where the device is known: on the handle for the HiFi-GAN generator (HgMemo,
csrc/hifigan.hip) and for the planes attention of the FS2 handles (bsg_fs2midi::planes_lds, csrc/fs2.hip), once per device for the GEMM
launchers that have no handle (grant_lds_per_device, csrc/bsg_common.h).  Modelled on tests/test_gpu_form_census.py
test_second_device_takes_every_form: one process builds and runs on cuda:0, releases, builds and runs the same on cuda:1, and asks for equal
form strings and equal bits.

  * HiFi-GAN at (16, 512), padded and ragged: cdiv(8 T, 246) B >= 256, the smallest round shape at which stage 1's 64-channel pairs take NB2,
    whose LDS at K = 11, d = 5 is 2 x 306 x 144 = 88 128 B;
  * one bsg_gemm_h2w_ex call forced onto the 128-row tile with 7 taps (LDS 77 184 B);
  * one FS2 decode at B = 1, T = 96 on the planes attention (75 776 B).

Skipped on a box with one GPU.
"""
import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from tests import h2w_cases as hc
from tests.test_gpu_fs2_shapes import _make_fs2
from tests.test_gpu_h2w_forms import run as h2w_run
from tests.test_gpu_hifigan_shapes import _mel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')]
torch.set_grad_enabled(False)


def _both(run):
    """run(device) on cuda:0, then on cuda:1, each with its device current -> the two results."""
    out = []
    for index in (0, 1):
        dev = torch.device('cuda', index)
        with torch.cuda.device(dev):
            out.append(run(dev))
    return out


def test_hifigan_nb2_pairs_on_the_second_device():
    import bench
    B, T = 16, 512
    mel = torch.from_numpy(_mel(B, T))
    lens = [512, 511, 300, 1] + [512] * 12

    def run(dev):
        voc, _ = bench.build_vocoder(dev)
        outs = []
        for kw in ({}, {'lengths': lens}):
            y = voc(mel.to(dev), **kw)
            outs.append((voc.last_path(), y.cpu().numpy()))
        voc.release()
        return outs

    first, second = _both(run)
    assert 'rb0.2.2:pair_h2/NB2' in first[0][0].split(), first[0][0]      # K = 11, d = 5 on 64 channels: the launch that needs the grant
    assert first[1][0].split()[0] == 'ragged', first[1][0]
    for (p0, a0), (p1, a1) in zip(first, second):
        assert p0 == p1, (p0, p1)
        assert np.array_equal(a0, a1), p0


def test_h2w_128_row_tile_on_the_second_device():
    c = hc.Case(256, 256, 64, taps=7, batch=2)
    assert hc.form_ok(c, 7)
    ops = hc.operands(c)

    def run(dev):
        _, raw, form = h2w_run(c, ops, 7)
        return form, raw

    (f0, r0), (f1, r1) = _both(run)
    assert f0 == f1 == hc.FORMS[7], (f0, f1)
    assert set(r0) == set(r1) and all(np.array_equal(r0[k], r1[k]) for k in r0), f0


def test_fs2_planes_attention_on_the_second_device():
    inp = synth.synth_inputs(1, 10, 96, seed=5)

    def run(dev):
        m = _make_fs2().to(dev)
        d = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
        kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
        r = m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], None, None, None, None, infer=True, **kw)
        out = m.last_path(), r['mel_out'].cpu().numpy()
        m.release()
        return out

    (p0, a0), (p1, a1) = _both(run)
    assert any(t.startswith('dec.attn:planes/') for t in p0.split()), p0
    assert p0 == p1, (p0, p1)
    assert np.array_equal(a0, a1), p0
