"""CPU: what tests/test_gpu_ddpm_shapes.py rests on, checked before any kernel runs (tests/ddpm_cases.py, tools/ddpm_yardsticks.py,
tests/golden/ddpm_yardsticks.json).

  * the record names every case of ddpm_cases.all_cases(); a few small ones are computed again and must agree with it (the deviation to a
    factor of 4: it is rounding noise and another host's convolutions sum in another order; max |want| to 1e-3; the clamp share to 0.01),
    which ties the file to this oracle, these weights, these inputs and these draws;
  * the clamp caps (LOW 0.10, MID 0.20) hold over the whole file: the windows are where eps reaches x.  HIGH is exempt and must in fact be
    mostly clamped (> 0.5), which is what it is there for;
  * a planted error: 3e-4 (4e-4 x max |eps|) added to the float64 oracle's eps at each row's last frame, at one step of the window, moves
    the final x by more than the window's bar, for every one of the six steps of LOW and MID at 3 x 77.  So the bar catches an eps error
    of that size on a single edge frame, whichever step it happens in, the sigma = 0 step with the smallest gain (0.010) included;
  * the window loop is oracle.diffusion.ddpm_sample's: from t = 99 over 100 steps at 2 x 64 it returns the same bits."""
import numpy as np
import pytest
import torch

from oracle import diffnet as odn, diffusion as odf
from tests import ddpm_cases as dc
from tests import plms_cases as pc

torch.set_grad_enabled(False)


@pytest.fixture(scope='module')
def yard():
    return dc.load_yardsticks()


def test_every_case_is_recorded_and_has_a_bar(yard):
    for window, B, T, lens in dc.all_cases():
        rec = yard[window][dc.case_name(B, T, lens is not None)]
        assert len(rec['dev']) == 3 and rec['dev'][0] > 0 and max(rec['dev'][1:]) <= rec['dev'][0], (window, B, T, rec)
    assert set(yard) == set(dc.WINDOWS)
    for window in dc.WINDOWS:
        names = {dc.case_name(B, T, lens is not None) for w, B, T, lens in dc.all_cases() if w == window}
        assert set(yard[window]) == names, (window, 'tests/golden/ddpm_yardsticks.json is stale: tools/ddpm_yardsticks.py')
        print(f'{window}: bar {dc.bar(window, yard):.3e} over {len(names)} cases')
        assert 0 < dc.bar(window, yard) < 1e-5      # fp32 rounding over at most six steps, nothing else


def test_clamp_caps_hold_over_the_record(yard):
    for window, cap in dc.CLAMP_CAP.items():
        worst = max(yard[window], key=lambda k: yard[window][k]['clamp'])
        print(f"{window}: largest clamp share {yard[window][worst]['clamp']:.3f} ({worst}), cap {cap}")
        assert yard[window][worst]['clamp'] <= cap, (window, worst)
    for rec in list(yard['HIGH'].values()) + list(yard['T99'].values()):
        assert rec['clamp'] > 0.5, rec      # the clamp branch itself


@pytest.mark.parametrize('window,B,T', dc.TIE_CASES)
def test_record_is_this_oracle(window, B, T, yard, gd_sd):
    x, cond, noise = dc.inputs(window, B, T)
    want, shares = dc.reference(gd_sd, window, x, cond, noise, torch.float64)
    dev = pc.deviations(dc.reference(gd_sd, window, x, cond, noise, torch.float32)[0], want)
    rec = yard[window][dc.case_name(B, T)]
    print(f"yardstick {window} {B}x{T}: {dev[0]:.3e} now, {rec['dev'][0]:.3e} recorded; clamp {max(shares):.3f} / {rec['clamp']:.3f}")
    assert rec['dev'][0] / 4 <= dev[0] <= rec['dev'][0] * 4
    assert abs(float(np.abs(want).max()) - rec['max']) <= 1e-3 * rec['max']
    assert abs(max(shares) - rec['clamp']) <= 0.01
    if window in dc.CLAMP_CAP:
        assert max(shares) <= dc.CLAMP_CAP[window]
    assert len(shares) == dc.WINDOWS[window][1] == noise.shape[0]


@pytest.mark.parametrize('window', dc.SWEEP)
def test_bar_catches_an_eps_error_on_one_edge_frame(window, yard, gd_sd):
    B, T = dc.PLANT_SHAPE
    x, cond, noise = dc.inputs(window, B, T)
    want, _ = dc.reference(gd_sd, window, x, cond, noise, torch.float64)
    bar = dc.bar(window, yard)
    for k in range(dc.WINDOWS[window][1]):
        got, _ = dc.reference(gd_sd, window, x, cond, noise, torch.float64, plant=(k, dc.PLANT))
        whole, ends, _ = pc.deviations(got, want)
        print(f'{window} {B}x{T}: {dc.PLANT:g} planted in eps at step {k} (t = {dc.WINDOWS[window][0] - k}) moves x_final by {whole:.3e}; bar {bar:.3e}')
        assert ends == whole      # it shows where it was planted or downstream of it: within the row ends' window
        assert whole > bar, (window, k, whole, bar)


def test_window_loop_is_ddpm_sample(gd_sd):
    from bisinger_amd import synth
    rs = np.random.RandomState(11)
    rs.standard_normal((2, 1, 80, 64))
    cond = torch.from_numpy(rs.standard_normal((2, 256, 64)).astype(np.float32))
    noise = torch.from_numpy(synth.synth_noise(100, 2, 80, 64, seed=1))
    x_T = noise[0][:, None].contiguous()
    den = lambda x_, t_: odn.diffnet_forward(gd_sd, x_, t_, cond, 'denoise_fn.')
    want = odf.ddpm_sample(pc.schedule(100), den, x_T, noise[1:][:, :, None], 100)
    got, shares = dc.steps(gd_sd, x_T, cond, noise[1:], 99, 100, torch.float32)
    assert np.array_equal(got, want.double().numpy())
    print(f'clamp share from x_T ~ N(0, 1): t = 99 {shares[0]:.2f}, t = 90 {shares[9]:.2f}, t = 20 {shares[79]:.2f}, t = 0 {shares[99]:.2f}')
    assert shares[0] > 0.75 and shares[9] > 0.7 and shares[99] < 0.3      # why a check that starts at t = 99 sees so little of eps
