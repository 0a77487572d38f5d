"""CPU: the C-ABI library builds, loads, and exports every symbol include/bisinger_hip.h declares."""
import os
import re
import subprocess

from bisinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, 'include', 'bisinger_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(bsg_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    from bisinger_amd.build import build
    path = build(verbose=False)
    lib = _lib.load()
    assert lib.bsg_abi_version() == _lib.ABI_VERSION
    syms = header_symbols()
    assert len(syms) >= 10
    out = subprocess.check_output(['nm', '-D', '--defined-only', path], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for s in syms:
        assert s in exported, f'{s} declared in the header but not exported'
        assert hasattr(lib, s)
    # and the ctypes binding covers the header
    assert sorted(_lib.declared_symbols()) == syms


def test_hifigan_last_path_without_a_forward():
    """bsg_hifigan_last_path names launches; a null handle has made none (the GPU side: tests/test_gpu_hifigan_shapes.py)."""
    assert _lib.load().bsg_hifigan_last_path(None) == b'none'


def test_fs2_last_path_without_a_call():
    """bsg_fs2midi_last_path / bsg_fftden_last_path name launch forms; a null handle has launched nothing (the GPU side:
    tests/test_gpu_fs2_shapes.py)."""
    assert _lib.load().bsg_fs2midi_last_path(None) == b'none'
    assert _lib.load().bsg_fftden_last_path(None) == b'none'


def test_product_path_fails_loudly_without_library(monkeypatch, tmp_path):
    import pytest
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.BsgError):
        _lib.load()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'bisinger_amd')
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith('.py'):
                txt = open(os.path.join(dp, fn)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', txt, flags=re.M), fn


def test_create_refuses_channel_counts_other_than_256_with_a_message():
    """hparams['residual_channels'] / ['hidden_size'] other than 256 (no shipped config has one): BSG_EINVAL and a message naming the value at
    create, before any device call — checked here without a GPU ("Differences from the reference's surface")."""
    import ctypes
    from ctypes import POINTER, byref, c_void_p, cast
    lib = _lib.load()
    dummy = (c_void_p * 200)(*([1] * 200))
    h = c_void_p()
    cfg = _lib.DiffnetCfg(80, 384, 384, 20, 4, 1000)
    rc = lib.bsg_diffnet_create(byref(h), byref(cfg), cast(dummy, POINTER(c_void_p)), 170, c_void_p(1), None)
    assert rc != 0 and h.value is None
    msg = lib.bsg_last_error().decode()
    assert '384' in msg and '256' in msg, msg
    fcfg = _lib.Fs2Cfg(192, 65, 4, 4, 2, 9, 9, 80, 2, 3, 22, 8, 2002, 5000)
    rc = lib.bsg_fs2midi_create(byref(h), byref(fcfg), cast(dummy, POINTER(c_void_p)), 143, c_void_p(1), c_void_p(1), None)
    assert rc != 0 and h.value is None
    msg = lib.bsg_last_error().decode()
    assert '192' in msg and '256' in msg, msg


def test_gemm_ex_refuses_bad_descriptors_with_a_message():
    """bsg_gemm_ex (the test entry that reaches all of launch_gemm): every refusal is BSG_EINVAL with a message, before any device call —
    checked here without a GPU."""
    from ctypes import byref, c_char_p
    lib = _lib.load()

    def desc(**kw):
        d = _lib.GemmDesc(A=0x1000, B=0x2000, C=0x3000, M=8, N=8, K=8, lda=8, ldb=8, ldc=8, trans_b=1, taps=1, alpha=1.0, batch=1)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(d, force, *words):
        form = c_char_p()
        rc = lib.bsg_gemm_ex(byref(d) if d is not None else None, force, byref(form), None)
        assert rc == -22 and form.value is None, (rc, form.value)
        msg = lib.bsg_last_error().decode()
        assert msg.startswith('gemm_ex:') and all(w in msg for w in words), msg

    refused(None, 0, 'null descriptor')
    for name in 'ABC':
        refused(desc(**{name: None}), 0, 'null operand')
    for name in ('M', 'N', 'K', 'batch', 'taps'):
        refused(desc(**{name: 0}), 0, 'non-positive', f'{name}=0')
        refused(desc(**{name: -3}), 5, 'non-positive', f'{name}=-3')
    refused(desc(post_scale_n=0x4000), 0, 'post_scale_n', 'post_shift_n')
    refused(desc(post_shift_n=0x4000), 0, 'post_scale_n', 'post_shift_n')
    refused(desc(R=0x4000), 0, 'R without ldr')
    for force in (-1, 6):
        refused(desc(), force, 'force_form', str(force))
    # the alignment rule of the split / fast kernels: K, lda, ldb, the A / B strides multiples of 4, N too unless trans_b, 16-byte bases
    unaligned = [dict(K=6), dict(lda=9), dict(ldb=10), dict(sA=66), dict(sB=65), dict(sA2=2), dict(sB2=7), dict(sTapB=1),
                 dict(A=0x1004), dict(B=0x2008), dict(trans_b=0, N=6)]
    for kw in unaligned:
        for force in (1, 2, 3, 4):
            refused(desc(**kw), force, 'force_form', 'aligned')


def test_gemm_h2w_ex_refuses_bad_descriptors_and_forms_with_a_message():
    """bsg_gemm_h2w_ex (the test entry that reaches all of launch_gemm_h2w): a bad descriptor and a forced form the kernel is not built for
    are BSG_EINVAL with a message, before any device call — checked here without a GPU.  The struct is the header's, field for field."""
    from ctypes import byref, c_char_p
    lib = _lib.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bisinger_hip.h')).read(), flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\} bsg_h2w_desc;', src).group(1)
    names = [n.strip(' *') for decl in body.split(';') if decl.strip() for n in decl.strip().split(None, 2 if decl.strip().startswith('const') else 1)[-1].split(',')]
    assert names == [f[0] for f in _lib.H2wDesc._fields_], names

    def desc(**kw):
        d = _lib.H2wDesc(act=0x1000, lda_src=256, lda=256, w=0x2000, ts=0, rs=256, ks=1, rows=8, K=256, Wn=128, taps=1, act_is_a=1, batch=1,
                         C=0x3000, ldc=128, alpha=1.0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(d, force, *words):
        form = c_char_p()
        rc = lib.bsg_gemm_h2w_ex(byref(d) if d is not None else None, force, byref(form), None)
        assert rc == -22 and form.value is None, (rc, form.value)
        msg = lib.bsg_last_error().decode()
        assert msg.startswith('gemm_h2w') and all(w in msg for w in words), msg

    refused(None, 0, 'null descriptor')
    refused(desc(act=None), 0, 'null operand')
    refused(desc(w=None), 0, 'null operand')
    refused(desc(C=None), 0, 'no output')
    refused(desc(batch=0), 0, 'batch 0')
    refused(desc(batch=4, zdiv=3), 0, 'zdiv 3')
    for kw in (dict(rows=0), dict(Wn=100), dict(K=96), dict(taps=18), dict(lda=260), dict(lda=192)):
        refused(desc(**kw), 0, 'unsupported shape')
    for kw in (dict(lda_src=258), dict(sAct_src=2), dict(act=0x1004)):
        refused(desc(**kw), 0, '16-byte aligned')
    refused(desc(batch=2, sAct=8), 0, 'plane batch stride')
    for force in (-1, 8):
        refused(desc(), force, 'force_form', str(force))
    for force in (1, 2, 3, 4):
        refused(desc(act_is_a=0), force, 'force_form', '32-row')
    refused(desc(taps=3, tap_shift0=-1), 1, 'force_form 1', 'plain product')
    refused(desc(K=128, lda=128), 1, 'force_form 1', 'K=128')
    refused(desc(K=64, lda=64), 3, 'ring of 8', 'does not divide')           # 4 k-steps
    refused(desc(K=64, lda=64, taps=3), 2, 'ring of 16', 'does not divide')  # 12 k-steps
    refused(desc(K=64, lda=64, taps=3, act_is_a=0), 5, 'ring of 8', 'does not divide')
    for force, taps in ((3, 1), (4, 1), (6, 1), (2, 1), (1, 9), (3, 9), (4, 9), (6, 9)):
        refused(desc(lens=0x4000, taps=taps), force, 'lengths', 'ragged') if not (force == 1 and taps == 9) else refused(desc(lens=0x4000, taps=taps), force, 'force_form 1')
