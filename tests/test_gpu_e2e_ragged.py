"""GPU: ragged forward_batch end to end — DiffSingerE2EInfer.forward_batch(items, seed=77, max_sentences=3, denoise_c=0.1, ragged_front=True,
ragged=True, ragged_pitch=True, ragged_vocoder=True) against the float64 "alone" chain of tests/e2e_ragged_cases.py: every item is what the
pipeline gives for that utterance alone (B = 1 on its own tokens and frames) with the draws of its row place in its bucket.  The stages
have thorough tests of their own; this file looks at what lies BETWEEN them (infer._generate_wavs, forward_batch,
GaussianDiffusion._forward_infer): the n_frames list three stages take as lengths, mel.transpose(2, 1), which f0 reaches the NSF source, the
seed of the NSF draws, lengths=[n * hop] of the post-filter, the Philox index of a ragged row's sampler noise, the bucket permutation, and
whether the durations predicted inside a ragged bucket are those of the utterance alone.

Two set-ups: `plain` (the workdir fixture of tests/test_gpu_infer.py: HiFi-GAN, no pitch extractor) and `nsf` (the nsf_workdir fixture of
tests/test_gpu_pe_ragged.py: pe_enable + use_nsf), both with the duration bias raised in the checkpoint (e2e_ragged_cases.raise_checkpoint).
Five items of 29, 135, 64, 81 and 65 frames; buckets [4, 1, 2] (T = 135) and [3, 0] (T = 81).

  a. the wiring is the stages: forward_batch's waveform of every item equals, bit for bit, the final output of stages() — collate,
     infer.model(ragged, ragged_front, seed), infer.pe(lengths), infer.vocoder(lengths, seed), vocoders.denoise(lengths) called in order per
     bucket; last_batch_stats['frames'] are the float64 chain's alone frame counts; n x hop samples each;
  b. every stage against float64 on the row alone, FED the device's previous stage output (hand-off):
        front            decoder_inp    fs2_ragged_cases.BOUND['decoder_inp'] (the project's bar of the ragged front, unchanged); mel2ph exact
        sampler          mel_out        4 x YARD_HANDOFF['mel_out'] (no project bar for these weights: 4 x the float32 oracle's own deviation)
        pitch extractor  pitch_pred, f0 _check_pitch of tests/test_gpu_f2_fullsize.py, the bar of tests/test_gpu_pe_ragged.py, unchanged: 2 x the
                                        float32 oracle's deviation + 2e-5 of the scale; frames whose voicing logit is within 10 bars of zero may
                                        fall either way, are left out of f0 only and capped at fs2_ragged_cases.TIE_CAP of a row
        vocoder          wav            BAR of tests/test_gpu_hifigan_shapes.py (5.4e-6; tests/test_gpu_hifigan_ragged.py holds the NSF generator
                                        to the same), whole row and separately the first and last hop samples
        post-filter      wav_denoised   bound((512, 128, 512)) of tests/test_gpu_wavden.py: 4 x err_fp32 of the triple, unchanged
     every one x max(1, max |want|); every float output exactly 0 beyond n (the waveforms beyond n x hop), mel2ph 0 beyond n;
  c. the composed result against the float64 chain with NO device hand-off: mel_out in both set-ups, the waveform before and after the
     post-filter (NSF set-up: the chain fed the device's f0, as the sine source integrates f0); bar 4 x YARD_COMPOSED.  A wrong Philox index
     of a ragged row moves mel_out by order 1;
  d. the five items in another order: every waveform bit-identical;
  e. one item alone (the shortest and the longest) through forward_batch([item], every switch) — B = 1 on the ragged kernels — and through
     forward_model(item, seed=77) — B = 1 on the padded kernels: both at row place 0 with T = n, held to alone_chain(b=0, B=1, T=n) at the bars
     of c; the difference between the two paths is printed, not asserted;
  f. no range event, no retry; denoise_fn.last_path() is stack_h2q_ragged_tail; fs2.last_path() holds esm:alone, tok:ragged, dec.ragged.

Yardsticks (tests/test_e2e_ragged_cpu.py, float32 alone_chain against float64, largest over the five items; x max(1, max |want|), f0 relative):
    hand-off   plain: decoder_inp 2.64e-7  mel_out 6.80e-7  wav 1.04e-6  wav_denoised 1.94e-7
               nsf:   decoder_inp 2.64e-7  mel_out 6.80e-7  pitch_pred 3.31e-6  f0 3.20e-6  wav 1.46e-6  wav_denoised 3.14e-7
    composed   plain: mel_out 7.69e-7  wav 1.13e-6  wav_denoised 1.10e-6
               nsf (float64 f0 fed): mel_out 7.69e-7  wav 1.49e-6  wav_denoised 1.44e-6
The float64 references are the cost (12 sampler runs of 100 denoiser evaluations on the CPU, about 5 s each); they are cached per
(set-up, item) and shared by the tests.

Measured on the MI355X (largest over the rows, normalised like the yardstick; in brackets the ratio to the recorded float32 yardstick;
every row of both set-ups passed, no range event):
    b, hand-off   plain: decoder_inp 3.57e-7 (1.27; bar 2.63e-6)  mel_out 8.59e-7 (1.21; bar 2.84e-6)  wav 1.10e-6 (1.00; bar 5.4e-6), its
                         edges 7.93e-7  wav_denoised 7.94e-7 (3.97; bar 5.09e-6)
                  nsf:   decoder_inp, mel_out as plain (the same bits)  pitch_pred 6.98e-6 absolute (bars 4.6e-5 .. 6.4e-5)  f0 4.11e-6 (1.25;
                         bars 3.3e-5 .. 4.5e-5), no near tie  wav 1.75e-6 (1.09; bar 5.4e-6), its edges 9.72e-7  wav_denoised 1.77e-6 (5.36; bar 5.09e-6)
    c, composed   plain: mel_out 7.87e-7 (0.98; bar 3.2e-6)  wav 1.26e-6 (1.05; bar 4.8e-6)  wav_denoised 1.22e-6 (1.02; bar 4.8e-6)
                  nsf:   mel_out 7.87e-7 (0.98; bar 3.2e-6)  wav 1.76e-6 (1.10; bar 6.4e-6)  wav_denoised 1.85e-6 (1.23; bar 6.0e-6)
    e, alone      plain: ragged path 1.21e-6, padded path 1.26e-6 (bar 4.8e-6); the two paths differ by 8.3e-7 (n = 29) and 8.8e-7 (n = 135)
                  nsf:   ragged path 1.64e-6 (bar 6.0e-6), padded path 1.49e-6 (bar 6.4e-6); the two paths differ by 1.0e-6 and 1.7e-6
The post-filter's hand-off figure is several times its yardstick on these waveforms (max |wav| about 0.1: few bins above the threshold) and
well inside the triple's bar, which comes from louder cases.

Planted once each, then reverted: n_frames off by one in _generate_wavs -> a, c, e fail; two rows' waveforms swapped in forward_batch ->
a, c; the padded T x hop as the post-filter's length -> a, c; every row's x_T drawn at row place 0 -> b (sampler), c.  What the tests
exposed: forward_model(item, seed=s) keyed the sampler by s but the NSF source's draws by hparams['seed'] (e failed in the NSF set-up);
it now passes the seed on, as forward_batch does.
"""
import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from oracle import pe as ope
from tests import e2e_ragged_cases as E
from tests import fs2_ragged_cases as RC
from tests.test_gpu_ddpm_shapes import _limit
from tests.test_gpu_f2_fullsize import _check_pitch
from tests.test_gpu_hifigan_shapes import BAR, EDGE
from tests.test_gpu_infer import workdir  # noqa: F401  (the synthetic checkpoint directory of the inference tests)
from tests.test_gpu_pe_ragged import nsf_workdir  # noqa: F401  (the pe_enable + use_nsf set-up)
from tests.test_gpu_wavden import bound as wavden_bound

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
HOP = E.HOP
CALL_LIMIT, REF_LIMIT = 120, 600      # seconds before the watchdog ends the process (tests/test_gpu_ddpm_shapes._limit)
ORDER = (2, 4, 0, 3, 1)               # another order of the five items (d)

_DEV = {}      # set-up -> everything the device computed (numpy), once
_REF = {}      # (kind, set-up, item) -> float64 chain


def switches(setup):
    kw = dict(ragged_front=True, ragged=True, ragged_vocoder=True)
    if setup == 'nsf':
        kw['ragged_pitch'] = True
    return kw


def stages(infer, bucket_items, seed):
    """The public pieces in the order _generate_wavs calls them, every intermediate kept (device tensors at the padded shapes)."""
    from bisinger_amd import vocoders
    from bisinger_amd.hparams import hparams
    sample = infer.collate(bucket_items)
    out = infer.model(sample['txt_tokens'], spk_embed=sample['spk_ids'], ref_mels=None, infer=True, pitch_midi=sample['pitch_midi'],
                      midi_dur=sample['midi_dur'], is_slur=sample['is_slur'], lang=sample['lang'], speechsing=sample['speechsing'], seed=seed,
                      ragged=True, ragged_front=True)
    mel, mel2ph = out['mel_out'], out['mel2ph']
    n = [int(v) for v in (mel2ph > 0).sum(-1).tolist()]
    r = {'decoder_inp': out['decoder_inp'], 'mel2ph': mel2ph, 'mel_out': mel, 'n': n}
    if hparams.get('use_nsf'):
        p = infer.pe(mel, lengths=n)
        r.update(pitch_pred=p['pitch_pred'], f0=p['f0_denorm_pred'])
        wav = infer.vocoder(mel.transpose(2, 1), r['f0'], seed=seed, lengths=n)[:, 0]
    else:
        wav = infer.vocoder(mel.transpose(2, 1), lengths=n)[:, 0]
    r['wav'] = wav
    r['wav_denoised'] = vocoders.denoise(wav.contiguous(), v=E.DENOISE_C, lengths=[v * HOP for v in n])
    return r


def device(setup, request):
    """Every device call of this file for one set-up, once: forward_batch, stages per bucket, forward_batch in another order, and the two
    lone items on both paths.  Nothing here compares values; the tests do."""
    if setup in _DEV:
        return _DEV[setup]
    request.getfixturevalue('workdir' if setup == 'plain' else 'nsf_workdir')
    from bisinger_amd.hparams import hparams, set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    E.raise_checkpoint('checkpoints/exp_diff_e2e/model_ckpt_steps_1000.ckpt')
    set_hparams('exp.yaml' if setup == 'plain' else 'exp2.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=4321')
    assert (hparams['fft_size'], hparams['hop_size'], hparams['win_size']) == E.TRIPLE and hparams['timesteps'] == E.STEPS
    infer = DiffSingerE2EInfer(hparams)
    assert int(np.prod(infer.vocoder.h['upsample_rates'])) == HOP
    sds = E.state_dicts(setup)
    # the checkpoint the device loaded is the state dict the chain reads
    msd = {k: v.detach().cpu() for k, v in infer.model.state_dict().items()}
    differ = [k for k, v in sds['model'].items() if k not in msd or not torch.equal(msd[k].reshape(-1), v.reshape(-1))]
    assert not differ, differ[:5]
    if setup == 'nsf':
        psd = {k: v.detach().cpu() for k, v in infer.pe.state_dict().items()}
        assert all(torch.equal(psd[k].reshape(-1), v.reshape(-1)) for k, v in sds['pe'].items())
    items = E.items()
    kw = dict(seed=E.SEED, max_sentences=E.MAX_SENTENCES, denoise_c=E.DENOISE_C, **switches(setup))
    d = {'retries': _lib.range_retries}
    with _limit(CALL_LIMIT):
        d['wavs'] = infer.forward_batch(items, **kw)
        d['stats'] = dict(infer.last_batch_stats)
        d['paths'] = (infer.model.denoise_fn.last_path(), infer.model.fs2.last_path().split())
        d['buckets'] = []
        for bk in d['stats']['buckets']:
            r = stages(infer, [items[i] for i in bk], E.SEED)
            d['buckets'].append({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()})
        again = infer.forward_batch([items[i] for i in ORDER], **kw)
        d['reordered'] = {i: w for i, w in zip(ORDER, again)}
        d['lone'] = {}
        f0s = []
        if setup == 'nsf':
            inner = infer.pe.forward

            def recording(mel, *a, **k):
                out = inner(mel, *a, **k)
                f0s.append(out['f0_denorm_pred'][0].cpu().numpy())
                return out
            infer.pe.forward = recording
        for i in (int(np.argmin(E.FRAMES)), int(np.argmax(E.FRAMES))):
            rag = infer.forward_batch([items[i]], seed=E.SEED, denoise_c=E.DENOISE_C, **switches(setup))[0]
            rag_frames, rag_path = infer.last_batch_stats['frames'][0], infer.model.denoise_fn.last_path()
            pad = infer.forward_model(items[i], seed=E.SEED)
            keep = list(f0s)
            unfiltered = infer.forward_batch([items[i]], seed=E.SEED, **switches(setup))[0]      # (for the printed difference of the two paths)
            d['lone'][i] = dict(ragged=rag, padded=pad, unfiltered=unfiltered, frames=rag_frames, path=rag_path, f0=keep)
            del f0s[:]
        if setup == 'nsf':
            infer.pe.forward = inner
        torch.cuda.synchronize()
    d['retries_after'] = _lib.range_retries
    d['events'] = (_lib.gemm_range_peek(), infer.vocoder.gemm_range_peek(), infer.model.fs2.gemm_range_peek(), infer.model.denoise_fn.gemm_range_peek(),
                   infer.pe.gemm_range_peek() if setup == 'nsf' else 0)
    net = infer.model.denoise_fn
    d['demoted'] = [a for a in ('_h2q_range_off', '_h2_range_off', 'split_disabled', 'parts_disabled') if getattr(net, a, False)]
    _DEV[setup] = d
    return d


def rows(d):
    """(item index, bucket record, row place b, B, T, n) of every row of both buckets."""
    for bk, r in zip(d['stats']['buckets'], d['buckets']):
        T = int(r['mel_out'].shape[1])
        for b, i in enumerate(bk):
            yield i, r, b, len(bk), T, r['n'][b]


def ref_handoff(setup, i, r, b, B, T, n):
    """The float64 chain of item i, every stage fed the device's previous stage output."""
    key = ('handoff', setup, i)
    if key not in _REF:
        feed = {'decoder_inp': r['decoder_inp'][b, :n], 'mel_out': r['mel_out'][b, :n], 'wav': r['wav'][b, :n * HOP]}
        if setup == 'nsf':
            feed['f0'] = r['f0'][b, :n]
        with _limit(REF_LIMIT):
            _REF[key] = E.alone_chain(E.state_dicts(setup), E.items()[i], b, B, T, E.SEED, F64, feed=feed)
    return _REF[key]


def ref_composed(setup, i, b, B, T, f0=None, tag=''):
    """The float64 chain of item i with no device hand-off (NSF set-up: the device's f0 fed to the sine source)."""
    key = ('composed' + tag, setup, i)
    if key not in _REF:
        with _limit(REF_LIMIT):
            _REF[key] = E.alone_chain(E.state_dicts(setup), E.items()[i], b, B, T, E.SEED, F64, feed=None if f0 is None else {'f0': f0})
    return _REF[key]


def show(tag, what, dev, bar, yard=None):
    print(f'  {tag} {what}: device {dev:.2e}  bar {bar:.2e}' + ('' if yard is None else f'  fp32 yardstick {yard:.2e} (x {dev / yard:.2f})'))


# ------------------------------------------------------------------------------------------------------------------
# a. the wiring is the stages
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setup', E.SETUPS)
def test_forward_batch_is_its_stages(setup, request):
    d = device(setup, request)
    st = d['stats']
    assert tuple(map(tuple, st['buckets'])) == E.BUCKETS
    assert tuple(st['frames']) == E.FRAMES, 'the durations predicted in a ragged bucket are not those of the utterance alone'
    seen = set()
    for i, r, b, B, T, n in rows(d):
        seen.add(i)
        assert n == E.FRAMES[i] and T == max(r['n'])
        assert d['wavs'][i].shape == (n * HOP,) and d['wavs'][i].dtype == np.float32
        assert np.array_equal(d['wavs'][i], r['wav_denoised'][b, :n * HOP]), f'item {i}: forward_batch is not its stages'
    assert seen == set(range(5))


# ------------------------------------------------------------------------------------------------------------------
# b. every stage against float64 on the row alone, fed the device's previous stage
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setup', E.SETUPS)
def test_every_stage_against_float64_on_the_row_alone(setup, request):
    d = device(setup, request)
    sds = E.state_dicts(setup)
    yard = E.YARD_HANDOFF[setup]
    wbound = wavden_bound(E.TRIPLE)
    bad = []
    for i, r, b, B, T, n in rows(d):
        tag = f'{setup} item {i} (row {b} of {B}, n={n}, T={T})'
        print(tag)
        want = ref_handoff(setup, i, r, b, B, T, n)
        assert want['n'] == n
        # zeros beyond the row's end
        for k in ('decoder_inp', 'mel_out', 'pitch_pred', 'f0', 'mel2ph'):
            if k in r:
                assert not r[k][b, n:].any(), (tag, k, 'not 0 beyond n')
        assert not r['wav'][b, n * HOP:].any() and not r['wav_denoised'][b, n * HOP:].any(), (tag, 'waveform not 0 beyond n x hop')
        # front
        assert np.array_equal(r['mel2ph'][b, :n], want['mel2ph']), (tag, 'mel2ph')
        fig = [('decoder_inp', E.norm_dev(r['decoder_inp'][b, :n], want['decoder_inp']), RC.BOUND['decoder_inp']),
               ('mel_out', E.norm_dev(r['mel_out'][b, :n], want['mel_out']), 4 * yard['mel_out'])]
        # vocoder: the whole row, and its first and last hop
        g, w = r['wav'][b, :n * HOP], want['wav']
        fig.append(('wav', E.norm_dev(g, w), BAR))
        scale = max(1.0, float(np.abs(w).max()))
        fig.append(('wav_edges', max(float(np.abs(g[:EDGE] - w[:EDGE]).max()), float(np.abs(g[-EDGE:] - w[-EDGE:]).max())) / scale, BAR))
        fig.append(('wav_denoised', E.norm_dev(r['wav_denoised'][b, :n * HOP], want['wav_denoised']), wbound))
        for what, dev, bar in fig:
            show(tag, what, dev, bar, yard[what.replace('_edges', '')])
            if not dev <= bar:
                bad.append((tag, what, dev, bar))
        if setup == 'nsf':
            # the pitch extractor on the device's mel of this row alone: _check_pitch's own bar and voicing rule
            mel = np.ascontiguousarray(r['mel_out'][b:b + 1, :n])
            got = {'pitch_pred': torch.from_numpy(r['pitch_pred'][b:b + 1, :n]), 'f0_denorm_pred': torch.from_numpy(r['f0'][b:b + 1, :n])}
            _check_pitch(tag, got, sds['pe'], mel, [n])
            p32 = ope.pitch_extractor_forward(sds['pe'], torch.from_numpy(mel), dtype=F32)['pitch_pred'][0].numpy()
            bar, tie = E.uv_margin(want['pitch_pred'], p32)
            assert float(tie.sum()) <= RC.TIE_CAP * n, (tag, 'voicing logits within the bar of zero', int(tie.sum()))
            show(tag, 'pitch_pred (absolute)', float(np.abs(r['pitch_pred'][b, :n] - want['pitch_pred']).max()), bar, yard['pitch_pred'])
            show(tag, f'f0 (relative, {int(tie.sum())} near ties left out)', E.f0_dev(r['f0'][b, :n], want['f0'], tie), 2 ** bar - 1 + 1e-6, yard['f0'])
            assert np.array_equal((r['f0'][b, :n] > 0)[~tie], (want['f0'] > 0)[~tie])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------
# c. the composed result against the float64 chain with no device hand-off
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setup', E.SETUPS)
def test_composed_result_against_the_float64_chain(setup, request):
    d = device(setup, request)
    yard = E.YARD_COMPOSED[setup]
    assert 4 * yard['wav'] <= (5e-3 if setup == 'nsf' else 2e-3) and 4 * yard['wav_denoised'] <= (5e-3 if setup == 'nsf' else 2e-3)
    bad = []
    for i, r, b, B, T, n in rows(d):
        tag = f'{setup} item {i} (row {b} of {B}, n={n}, T={T})'
        want = ref_composed(setup, i, b, B, T, r['f0'][b, :n] if setup == 'nsf' else None)
        assert want['n'] == n
        for what, got in (('mel_out', r['mel_out'][b, :n]), ('wav', r['wav'][b, :n * HOP]), ('wav_denoised', d['wavs'][i])):
            dev = E.norm_dev(got, want[what])
            show(tag, what, dev, 4 * yard[what], yard[what])
            if not dev <= 4 * yard[what]:
                bad.append((tag, what, dev, 4 * yard[what]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------
# d. the order of the items does not matter
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setup', E.SETUPS)
def test_item_order_does_not_matter(setup, request):
    d = device(setup, request)
    assert list(ORDER) != sorted(ORDER)
    for i in range(5):
        assert np.array_equal(d['reordered'][i], d['wavs'][i]), f'item {i} changed with the order of the items'


# ------------------------------------------------------------------------------------------------------------------
# e. one item alone, on both paths
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setup', E.SETUPS)
def test_one_item_alone_on_both_paths(setup, request):
    d = device(setup, request)
    yard = E.YARD_COMPOSED[setup]
    bad = []
    for i, lone in d['lone'].items():
        n = E.FRAMES[i]
        tag = f'{setup} item {i} alone (n={n})'
        assert lone['frames'] == n and lone['ragged'].shape == lone['padded'].shape == (n * HOP,)
        assert lone['path'] == 'stack_h2q_ragged_tail', lone['path']
        if setup == 'nsf':
            assert len(lone['f0']) == 2 and all(f.shape == (n,) for f in lone['f0'])
        for k, (path, what) in enumerate((('ragged', 'wav_denoised'), ('padded', 'wav'))):
            want = ref_composed(setup, i, 0, 1, n, lone['f0'][k] if setup == 'nsf' else None, tag=f'-lone-{path}')
            dev = E.norm_dev(lone[path], want[what])
            show(tag, f'{path} path, {what}', dev, 4 * yard[what], yard[what])
            if not dev <= 4 * yard[what]:
                bad.append((tag, path, what, dev, 4 * yard[what]))
        print(f'  {tag}: forward_model against forward_batch([item]) without the post-filter: {E.norm_dev(lone["padded"], lone["unfiltered"]):.2e}')
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------
# f. no range event and no retry
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setup', E.SETUPS)
def test_no_range_event_and_the_ragged_paths(setup, request):
    d = device(setup, request)
    assert d['retries_after'] == d['retries'] and not any(d['events']) and not d['demoted'], (d['retries'], d['retries_after'], d['events'], d['demoted'])
    den, fs2 = d['paths']
    assert den == 'stack_h2q_ragged_tail', den
    assert 'esm:alone' in fs2 and 'tok:ragged' in fs2 and 'dec.ragged' in fs2, fs2
