"""The launch plan of the FFT stack (plan_fft, csrc/fs2.hip) chooses what the recorded commit chose, token for token.

tests/golden/fs2_paths.json holds bsg_fs2midi_last_path / bsg_fftden_last_path as the parent commit of the plan refactor wrote them
(tools/make_golden_fs2_paths.py run against that commit's build; its commit id and the digest of its library are in the file).  Here the
FastSpeech2MIDI of tests/test_gpu_fs2_shapes.py runs GRID on the default switches in one process, each case an encode followed by the
forward, and every string must equal the record; tests/test_gpu_fs2_shapes.py compares the switch sets (`forms`) and the FFT denoiser
(`den`) on the runs it makes anyway.  The strings depend on the shapes and the constants of csrc/fs2.hip only, not on the box.

GRID sits at the plan's own edges (2 heads; the encoder stack runs B x T_txt rows, the decoder stack B x T):
  B T = 31 | 32 rows and Tp <= 3 T (T = 10 | 11): the planes attention starts;
  Tp / 32 = 7 | 8 blocks (T = 224 | 225) and 15 | 16 blocks (T = 480 | 481): the second and the fourth key split start;
  ceil(T / 64) B heads = 128 | 129 and 256 | 257 (T = 1000: B = 4 | 5 and 8 | 9): the fourth and the second key split end;
  T % 32 in {0, 1, 31}.
With T_txt = max(1, T // 10) the encoder never has the 16 key blocks that four splits ask for (T_txt <= 250: 8 blocks), so EXTRA adds
T_txt = 480 | 481 (15 | 16 blocks) at T = 1000, as C(1, 481, 1000) of tests/test_gpu_fs2_shapes.py does.

So that a thin grid cannot hide a lost branch, the record itself is checked first (no GPU needed): over `default` both stacks show
split/nw2 and the planes attention on 1, 2 and 4 key splits, and both QKV producers of the pre-split path; over `forms` the union shows the
four-wave forms, the fp32-pipe forms, the score tensor, eight key splits, the other two QKV producers and the ESM's thread kernel.
"""
import pytest
import torch

from tests import util

GRID_B = [1, 2, 3, 4, 5, 8, 9, 16, 64]
GRID_T = [1, 5, 10, 11, 31, 32, 33, 224, 225, 257, 480, 481, 512, 993, 1000, 1001, 2500]
EXTRA = [(1, 480, 1000), (1, 481, 1000), (2, 481, 1000)]      # the encoder at 15 | 16 key blocks: its fourth key split
GRID = [(B, max(1, T // 10), T) for B in GRID_B for T in GRID_T if B * T <= 16016] + EXTRA      # (B, T_txt, T)


def key(B, Tt, T):
    return f'{B}x{Tt}x{T}'


def load_golden():
    return util.load_golden('fs2_paths.json')


def _site_forms(paths):
    """site -> the set of forms it shows over `paths`."""
    seen = {}
    for p in paths:
        for tok in p.split():
            site, form = tok.split(':')
            seen.setdefault(site, set()).add(form)
    return seen


def check_record(gold):
    assert set(gold['default']) == {key(*c) for c in GRID}
    seen = _site_forms(gold['default'].values())
    for st in ('enc', 'dec'):
        assert {'split/nw2', 'planes/ks1', 'planes/ks2', 'planes/ks4'} <= seen[f'{st}.attn'], (st, seen[f'{st}.attn'])
        assert {'fused', 'h2w'} <= seen[f'{st}.qkv'], (st, seen[f'{st}.qkv'])
    forms = _site_forms(p for case in gold['forms'].values() for p in case.values())
    attn = forms['enc.attn'] | forms['dec.attn']
    assert {'split/nw4', 'flash/nw2', 'flash/nw4', 'softmax', 'planes/ks8'} <= attn, attn
    assert {'split_kernel', 'gemm'} <= forms['enc.qkv'] | forms['dec.qkv'], forms
    assert 'thread' in forms['esm'], forms['esm']
    assert gold['den'] and all(t.startswith('den.') for p in gold['den'].values() for t in p.split())


def test_record_reaches_every_branch():
    check_record(load_golden())


@pytest.mark.gpu
def test_plan_chooses_what_the_parent_chose():
    from bisinger_amd import synth
    from tests import test_gpu_fs2_shapes as S
    gold = load_golden()
    check_record(gold)
    torch.set_grad_enabled(False)
    m = S._make_fs2()
    differ = []
    for B, Tt, T in sorted(GRID, key=lambda c: -c[0] * c[2]):      # largest first: the workspaces grow once
        d = {k: torch.from_numpy(v).cuda() for k, v in synth.synth_inputs(B, Tt, T, seed=5).items()}
        kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
        m.encode(d['txt_tokens'], d['spk_embed'], **kw)
        m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], None, None, None, None, infer=True, **kw)
        assert m.gemm_range_peek() == 0, (B, Tt, T, 'a range event fired: last_path would name the repeat')
        path = m.last_path()
        if path != gold['default'][key(B, Tt, T)]:
            differ.append((B, Tt, T, path, gold['default'][key(B, Tt, T)]))
    m.release()
    assert not differ, (len(differ), differ[:3])
