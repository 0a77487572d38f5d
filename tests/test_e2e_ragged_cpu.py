"""CPU: the items, the "alone" chain and the yardsticks of the end-to-end ragged test (tests/e2e_ragged_cases.py; the GPU side is
tests/test_gpu_e2e_ragged.py).

  1. the item conditions of tests/e2e_ragged_cases.py, evaluated again with the float64 front: a failure names the item and the condition;
  2. alone_chain in float32 at (b = 0, B = 1, T = n) equals the padded oracle composition of tests/test_gpu_infer.py on the same lone item
     bit for bit (_oracle_wav itself in the plain set-up; the steps of test_e2e_with_pitch_extractor_and_nsf_vocoder in the NSF one): the
     chain adds no arithmetic;
  3. the yardsticks: per set-up and stage the largest deviation of the float32 alone_chain from the float64 one over the five items at their
     row places, in hand-off mode (every float32 stage FED the float64 previous stage) and composed (no feed); normalised x max(1, max |want|),
     f0 relative to max(1, f0).  Each figure is held to the one recorded in e2e_ragged_cases.YARD_HANDOFF / YARD_COMPOSED, from which the GPU
     test takes 4 x; the voicing logits of the float64 chain within the pitch extractor's bound of zero stay under TIE_CAP of every row.

The float64 and float32 samplers are the cost: 17 runs of 100 denoiser evaluations, about 40 s on 16 threads."""
import types

import numpy as np
import pytest
import torch

from bisinger_amd import synth
from tests import e2e_ragged_cases as E
from tests import fs2_ragged_cases as RC
from tests import wavden_ref

torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
_FRONT = {}
_CHAINS = {}


def front():
    if not _FRONT:
        its = E.items()
        res = [E.front_only(it) for it in its]
        _FRONT.update(items=its, frames=[r[0] for r in res], xs=[r[1] for r in res])
    return _FRONT


def chains(setup):
    """Per item: the float64 chain at its place, the float32 chain fed the float64 stages, the float32 chain composed (NSF: fed f0 only)."""
    if setup not in _CHAINS:
        fr = front()
        sds = E.state_dicts(setup)
        place = E.places(fr['items'], fr['frames'])
        out = []
        for i, it in enumerate(fr['items']):
            at = place[i] + (E.SEED,)
            c64 = E.alone_chain(sds, it, *at, F64)
            feed = {k: c64[k] for k in ('decoder_inp', 'mel_out', 'wav')}
            if setup == 'nsf':
                feed['f0'] = c64['f0']
            h32 = E.alone_chain(sds, it, *at, F32, feed=feed)
            c32 = E.alone_chain(sds, it, *at, F32, feed={'f0': c64['f0']} if setup == 'nsf' else None)
            out.append((c64, h32, c32))
        _CHAINS[setup] = out
    return _CHAINS[setup]


def test_item_conditions():
    fr = front()
    est, bks = E.buckets(fr['items'])
    print(f'\nframes {fr["frames"]}  estimate_frames {est}  buckets {bks}')
    bad = E.conditions(fr['items'], fr['frames'], fr['xs'])
    assert not bad, bad
    assert tuple(fr['frames']) == E.FRAMES and tuple(map(tuple, bks)) == E.BUCKETS
    assert E.conditions(fr['items'][:4] + [fr['items'][0]], fr['frames'][:4] + [fr['frames'][0]], fr['xs'][:4] + [fr['xs'][0]])      # (it can fail)


@pytest.mark.parametrize('setup', E.SETUPS)
def test_chain_is_the_padded_oracle_composition(setup):
    from oracle import fs2 as ofs2, melgen as omg, nsf as onsf, pe as ope
    from tests.test_gpu_infer import _oracle_wav
    sds = E.state_dicts(setup)
    i = int(np.argmin(E.FRAMES))
    it, n, seed = E.items()[i], E.FRAMES[i], E.SEED
    got = E.alone_chain(sds, it, 0, 1, n, seed, F32)
    oin = E.lone_inputs(it)
    if setup == 'plain':
        infer = types.SimpleNamespace(model=types.SimpleNamespace(state_dict=lambda: sds['model']))
        sample = dict(oin, spk_ids=oin['spk_embed'])
        r, wav = _oracle_wav(infer, sample, seed, sds['voc'], {'hifigan_cfg': sds['voc_cfg']})
    else:
        f = ofs2.fs2_forward(sds['model'], oin)
        B, T = f['mel2ph'].shape
        cnt = B * 80 * T
        noise = np.stack([synth.philox_normal(seed, 0, cnt)] + [synth.philox_normal(seed, k + 1, cnt) for k in reversed(range(100))])
        r = omg.mel_gen(sds['model'], oin, torch.from_numpy(noise.reshape(101, B, 80, T)), fs2_out=f)
        p = ope.pitch_extractor_forward(sds['pe'], r['mel_out'])
        assert np.array_equal(got['pitch_pred'], p['pitch_pred'][0].numpy()) and np.array_equal(got['f0'], p['f0_denorm_pred'][0].numpy())
        ri = torch.from_numpy(np.random.RandomState(seed).uniform(size=(B, 9)).astype(np.float32))
        nz = torch.from_numpy(synth.philox_normal(seed, 0x4E5346, B * T * 256 * 9).reshape(B, T * 256, 9))
        wav = onsf.nsf_hifigan_forward(sds['voc'], r['mel_out'].transpose(1, 2), p['f0_denorm_pred'], ri, nz, sds['voc_cfg'])
    assert r['mel2ph'].shape == (1, n) and np.array_equal(got['mel2ph'], r['mel2ph'][0].numpy())
    assert np.array_equal(got['decoder_inp'], r['decoder_inp'][0].numpy())
    assert np.array_equal(got['mel_out'], r['mel_out'][0].numpy())
    assert got['wav'].dtype == np.float32 and np.array_equal(got['wav'], wav[0, 0].numpy())
    assert np.array_equal(got['wav_denoised'], wavden_ref.denoise(wav[0, 0].numpy(), E.DENOISE_C, *E.TRIPLE, dtype=np.float32))
    assert float(np.abs(got['wav_denoised'] - got['wav']).max()) > 1e-3      # the filter does something at this value


@pytest.mark.parametrize('setup', E.SETUPS)
def test_yardsticks(setup):
    fr = front()
    hand = dict.fromkeys(E.YARD_HANDOFF[setup], 0.0)
    comp = dict.fromkeys(E.YARD_COMPOSED[setup], 0.0)
    for it, n, (c64, h32, c32) in zip(fr['items'], fr['frames'], chains(setup)):
        assert c64['n'] == h32['n'] == c32['n'] == n
        assert np.array_equal(c64['mel2ph'], h32['mel2ph']) and np.array_equal(c64['dur_choice'], h32['dur_choice'])
        tie = None
        if setup == 'nsf':
            bar, tie = E.uv_margin(c64['pitch_pred'], h32['pitch_pred'])
            print(f'{it["item_name"]}: pitch bar {bar:.2e}, frames within 10 bars of the voicing edge {int(tie.sum())} of {n}, voiced {int((c64["f0"] > 0).sum())}')
            assert float(tie.sum()) <= RC.TIE_CAP * n, (it['item_name'], 'voicing logits near zero', int(tie.sum()), n)
            assert np.array_equal(c64['uv'][~tie], h32['uv'][~tie])
        for k in hand:
            d = E.f0_dev(h32[k], c64[k], tie) if k == 'f0' else E.norm_dev(h32[k], c64[k])
            hand[k] = max(hand[k], d)
        for k in comp:
            comp[k] = max(comp[k], E.norm_dev(c32[k], c64[k]))
    print(f'\n{setup} hand-off yardsticks (float32 stage fed the float64 previous stage, against float64): ' + '  '.join(f'{k} {v:.3e}' for k, v in hand.items()))
    print(f'{setup} composed yardsticks (float32 chain' + (' fed the float64 f0' if setup == 'nsf' else '') + ', against float64): '
          + '  '.join(f'{k} {v:.3e}' for k, v in comp.items()))
    for k, v in hand.items():
        assert v <= E.YARD_HANDOFF[setup][k], (setup, 'hand-off', k, v, E.YARD_HANDOFF[setup][k])
    for k, v in comp.items():
        assert v <= E.YARD_COMPOSED[setup][k], (setup, 'composed', k, v, E.YARD_COMPOSED[setup][k])
    # 4 x the composed yardstick must stay inside the project's end-to-end bars (tests/test_gpu_infer.py): beyond them the yardstick is suspect
    assert 4 * E.YARD_COMPOSED[setup]['wav'] <= (5e-3 if setup == 'nsf' else 2e-3)
