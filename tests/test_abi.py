"""The C ABI: include/strive_hip.h, the ctypes binding and the hipcc-built library stay in sync.  No compute
is issued here (there is no GPU in the build container); loading the library and resolving symbols is enough."""
import os
import re

import pytest

from strive_amd import _lib as L

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def header_functions():
    hdr = open(os.path.join(REPO, 'include', 'strive_hip.h')).read()
    return sorted(set(re.findall(r'\b(strive_[a-z0-9_]+)\s*\(', hdr)))


def test_binding_lists_every_header_symbol():
    assert header_functions() == sorted(L.PROTOTYPES.keys())


def test_hip_library_builds_loads_and_exports_everything():
    import __graft_entry__ as ge
    path = ge.build(verbose=False)
    assert os.path.exists(path)
    lib = L.StriveLib(path)            # raises if any symbol is missing
    assert lib.missing == []
    assert lib.query("strive_abi_version") == L.ABI_VERSION == 17


def test_library_reads_no_environment_variable():
    """ABI 17: every switch of the library is a declared option (strive_set_option); no getenv anywhere in csrc."""
    csrc = os.path.join(REPO, 'strive_amd', 'csrc')
    hits = []
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith(('.hip', '.h')):
            for i, line in enumerate(open(os.path.join(csrc, fn)), 1):
                code = line.split('//')[0]
                if re.search(r'\bgetenv\s*\(', code) or 'secure_getenv' in code:
                    hits.append('%s:%d' % (fn, i))
    assert hits == []


def test_options_are_declared_defaulted_and_range_checked(monkeypatch):
    import __graft_entry__ as ge
    lib = L.StriveLib(ge.build(verbose=False))
    names = lib.option_names()
    hdr = open(os.path.join(REPO, 'include', 'strive_hip.h')).read()
    assert len(names) == len(set(names)) >= 19
    for n in names:                                    # every option is documented in the header
        assert re.search(r'\b%s\b' % n, hdr), n
    lib.query('strive_reset_options')
    assert lib.get_option('conv_wsx') == 1 and lib.get_option('cnn_small_batch') == 96 and lib.get_option('sweep_step') == -1
    lib.set_option('cnn_small_batch', 0)
    assert lib.get_option('cnn_small_batch') == 0
    with pytest.raises(L.StriveHipError):
        lib.set_option('cnn_chunk', 4)                 # below the option's range
    with pytest.raises(L.StriveHipError):
        lib.set_option('no_such_option', 1)
    # the host maps STRIVE_<NAME> onto the options (and back to the defaults when the variable goes away)
    monkeypatch.setenv('STRIVE_SCENE_KERNELS', '0')
    lib.sync_options_from_env()
    assert lib.get_option('scene_kernels') == 0 and lib.get_option('cnn_small_batch') == 96
    monkeypatch.delenv('STRIVE_SCENE_KERNELS')
    lib.sync_options_from_env()
    assert lib.get_option('scene_kernels') == 1


def test_every_entry_point_cites_the_reference():
    hdr = open(os.path.join(REPO, 'include', 'strive_hip.h')).read()
    assert hdr.count('reference src/') >= 12


def test_product_has_no_cpu_path():
    import torch
    from strive_amd import ops
    with pytest.raises(L.StriveHipError):
        ops.map_crop(None, torch.zeros((1, 4)), torch.zeros((1,), dtype=torch.long))


def test_fused_conv1_entry_points_refuse_a_map_without_the_interleaved_raster():
    """conv1b_kernel<true> gathers from StriveMap.raster_px4 and from nothing else: every entry point that launches it returns an
    error for NULL before any launch (emulated library: a launch would dereference NULL on the host)."""
    import sys
    import torch
    from strive_amd import params, synth
    from util import product_model
    sys.path.insert(0, os.path.join(REPO, 'tests', 'hipemu'))
    import build as emu_build
    emu = L.StriveLib(emu_build.build(), require_all=True)
    raster, dx = synth.make_raster(512, 512)
    mp = params.pack_map(synth.SyntheticMapEnv(raster, dx), 'cpu')
    assert mp.struct.raster_px4
    mp.struct.raster_px4 = None
    cnn = params.pack_cnn(product_model()[1])
    n = 2
    fr = torch.tensor([[60.0, 60.0, 1.0, 0.0], [50.0, 70.0, 0.0, 1.0]])
    mi = torch.zeros((n,), dtype=torch.int32)
    z4, o4 = L.f4([0] * 4), L.f4([1] * 4)
    wsb = emu.query('strive_map_cnn_workspace_bytes', n)
    ws, feat = torch.zeros(wsb, dtype=torch.uint8), torch.full((n, 64), 7.0)
    kb = emu.query('strive_map_cnn_keep_bytes', n)
    kept = torch.zeros(kb, dtype=torch.uint8)
    npar = emu.query('strive_map_cnn_param_count')
    bwb = emu.query('strive_map_cnn_bwd_workspace_bytes', n)
    calls = [('strive_map_cnn_fwd', (mp.ref(), cnn.ref(), L.ptr(fr), z4, o4, L.ptr(mi), n, L.ptr(feat), L.ptr(ws), wsb, None)),
             ('strive_map_cnn_fwd_keep', (mp.ref(), cnn.ref(), L.ptr(fr), z4, o4, L.ptr(mi), n, L.ptr(feat), L.ptr(ws), wsb, L.ptr(kept), kb, n, 0, None)),
             ('strive_map_cnn_bench_layer', (mp.ref(), cnn.ref(), 0, L.ptr(fr), z4, o4, L.ptr(mi), n, L.ptr(feat), L.ptr(ws), wsb, None)),
             ('strive_map_cnn_bwd', (mp.ref(), cnn.ref(), L.ptr(fr), z4, o4, L.ptr(mi), n, L.ptr(torch.ones((n, 64))), L.ptr(torch.zeros(npar)),
                                     L.ptr(torch.zeros(bwb, dtype=torch.uint8)), bwb, None))]
    for name, args in calls:
        with pytest.raises(L.StriveHipError, match='raster_px4'):
            emu.call(name, *args)
    assert float(feat.min()) == 7.0 and not bool(ws.any()), 'nothing was launched'


def test_product_never_imports_the_oracle():
    import subprocess
    out = subprocess.run(['grep', '-rln', '--include=*.py', '-E', r'^\s*(from|import)\s+oracle', os.path.join(REPO, 'strive_amd')],
                         capture_output=True, text=True).stdout.strip()
    assert out == '', 'strive_amd imports oracle: %s' % out


def test_no_packed_fp32_ops_in_the_device_code():
    """MI355X returned wrong values in lanes 48-63 for v_pk_add_f32 with crossed op_sel halves when >= 4 waves shared
    a SIMD with MFMA-issuing neighbours (tools/pk_waw_probe.hip, profiles/r01_pk_add_opsel_probe.txt).  The library
    is therefore built without auto-formed packed fp32 arithmetic; this checks the disassembly of what was built."""
    from strive_amd import build
    counts = build.audit_packed_ops()
    if counts is None:
        pytest.skip('llvm-objdump not available')
    assert counts.get('_code_objects', 0) >= 1 and counts.get('_mfma', 0) > 0, 'no gfx950 code objects found: %r' % (counts,)
    packed = {k: v for k, v in counts.items() if not k.startswith('_')}
    assert not packed, 'packed fp32 VALU ops in the device code: %r' % (packed,)
