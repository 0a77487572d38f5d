"""The launch plan of the HiFi-GAN forward (plan_hifigan, csrc/hifigan.hip) chooses what the recorded commit chose, token for token.

tests/golden/hifigan_paths.json holds bsg_hifigan_last_path as the parent commit of the plan refactor wrote it (tools/make_golden_hifigan_paths.py
run against that commit's build; its commit id and the digest of its library are in the file).  Here the plain generator of bench.build_vocoder
runs GRID on the default switches in one process and every string must equal the record; tests/test_gpu_hifigan_shapes.py compares the
switch sets and the other generators on the runs it makes anyway.  The strings depend on the shapes and the thresholds only, not on the box.

So that a thin grid cannot hide a lost branch, the record itself is checked first (no GPU needed): both u = 2 stages show all three of
their forms, every 8- / 16-channel ResBlock both chain widths, every 32- / 64-channel pair both tile heights, and the `valu` switch set
two widths of the fused vector pair as well as the unfused pair.
"""
import json
import os

import pytest
import torch

from tests.util import ROOT

GRID_B = [1, 2, 3, 5, 8, 16, 64]
GRID_T = [1, 2, 3, 5, 8, 13, 21, 33, 55, 89, 127, 128, 129, 255, 256, 257, 413, 511, 512, 513, 683, 999, 1000, 1001, 1500, 2047, 2048, 2049, 2500,
          3001]
GRID = [(B, T) for B in GRID_B for T in GRID_T if B * T <= 16016]


def load_golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'hifigan_paths.json')) as f:
        return json.load(f)


def _site_forms(paths):
    """site -> the set of '<form>[/<variant>]' it shows over `paths`."""
    seen = {}
    for p in paths:
        for tok in p.split():
            site, form = tok.split(':')
            seen.setdefault(site, set()).add(form)
    return seen


def check_record(gold):
    assert set(gold['plain']) == {f'{B}x{T}' for B, T in GRID}
    seen = _site_forms(gold['plain'].values())
    for site in ('up2', 'up3'):
        assert {'up2', 'upk'} <= seen[site] and any(f.startswith('poly/') for f in seen[site]), (site, seen[site])
    for i in (2, 3):
        for j in range(3):
            assert {'chain/NC4', 'chain/NC8'} <= seen[f'rb{i}.{j}'], (i, j, seen[f'rb{i}.{j}'])
    for i in (0, 1):
        for j in range(3):
            for m in range(3):
                assert {'pair_h2/NB1', 'pair_h2/NB2'} <= seen[f'rb{i}.{j}.{m}'], (i, j, m, seen[f'rb{i}.{j}.{m}'])
    valu = set().union(*_site_forms(gold['forms']['valu'].values()).values())
    assert len({f for f in valu if f.startswith('pair_valu/TT')}) >= 2, valu
    assert any(f.startswith('conv1/') for f in valu) and any(f.startswith('conv2/') for f in valu), valu


def test_record_reaches_every_branch():
    check_record(load_golden())


@pytest.mark.gpu
def test_plan_chooses_what_the_parent_chose():
    import bench
    gold = load_golden()
    check_record(gold)
    torch.set_grad_enabled(False)
    voc, _ = bench.build_vocoder(torch.device('cuda', 0))
    differ = []
    for B, T in sorted(GRID, key=lambda s: -s[0] * s[1]):      # largest first: the stage buffers grow once
        mel = torch.randn(B, 80, T, device='cuda', generator=torch.Generator('cuda').manual_seed(1000 * B + T)) * 1.5 - 3.0
        voc(mel)
        got = voc.last_path()
        assert voc.gemm_range_peek() == 0, (B, T, 'a range event fired: last_path would name the repeat')
        if got != gold['plain'][f'{B}x{T}']:
            differ.append((B, T, got, gold['plain'][f'{B}x{T}']))
    assert not differ, (len(differ), differ[:3])
