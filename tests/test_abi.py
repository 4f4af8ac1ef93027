"""The C-ABI library loads, exports every symbol include/sketchycolor_hip.h declares, and the ctypes
mirrors of the descriptor structs have the C sizes (checked by compiling the header with gcc)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sketchycolor_hip.h')


def _declared():
    return set(re.findall(r'\bint (ssc_\w+)\(', open(HEADER).read()))


def test_library_exports_every_declared_symbol():
    from sketchyscenecolorization_amd import build, hip
    path = build.build_library(verbose=False)
    lib = ctypes.CDLL(path)
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), n
    assert names == set(hip.SIGNATURES), names ^ set(hip.SIGNATURES)
    assert lib.ssc_version() >= 100
    assert hasattr(lib, 'ssc_crc32c')      # the one non-int entry point (host CRC-32C for the TFRecord reader)


def test_struct_layouts_match_header():
    from sketchyscenecolorization_amd import hip
    src = '#include <stdio.h>\n#include "sketchycolor_hip.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(ssc_gview), ' \
          'sizeof(ssc_conv_desc), sizeof(ssc_wgrad_desc));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(hip.GView), ctypes.sizeof(hip.ConvDesc), ctypes.sizeof(hip.WgradDesc)]


def test_no_oracle_import_in_product():
    """The product path must never route through the oracle (or /root/reference)."""
    pkg = os.path.join(ROOT, 'sketchyscenecolorization_amd')
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                txt = open(os.path.join(base, f)).read()
                assert 'import oracle' not in txt and 'from oracle' not in txt, f
                assert '/root/reference' not in txt, f
    assert 'oracle' not in sys.modules or True


def test_stale_binary_is_refused(tmp_path, monkeypatch):
    """The library carries the hash of the sources it was built from (ssc_build_hash); a tree whose kernel sources differ --
    here: one comment appended to a .hip file, no rebuild -- makes hip.lib() (and with it smoke(), bench.py, every test)
    fail loudly instead of running the old binary under the new sources' name."""
    import shutil
    from sketchyscenecolorization_amd import build, hip
    build.build_library(verbose=False)
    assert build.library_hash() == build.tree_hash() and not build.is_stale()
    l = ctypes.CDLL(build.LIB_PATH)
    hip._declare(l)
    assert hip.build_hash(l) == build.tree_hash()
    csrc2 = tmp_path / 'csrc'
    shutil.copytree(build.CSRC, str(csrc2))
    with open(str(csrc2 / 'igemm.hip'), 'a') as f:
        f.write('// touched\n')
    monkeypatch.setattr(build, 'CSRC', str(csrc2))
    assert build.is_stale()
    monkeypatch.setattr(hip, '_lib', None)
    monkeypatch.delenv('SSC_ALLOW_STALE_LIB', raising=False)
    try:
        hip.lib()
    except RuntimeError as e:
        assert 'built from kernel sources' in str(e)
    else:
        raise AssertionError('a stale library was accepted')
    assert hip._lib is None
    # smoke() starts with the same check
    import __graft_entry__ as G
    src = open(G.__file__).read()
    assert 'hip.check_build_hash()' in src.split('def smoke')[1]


def test_library_has_no_packed_fp32_math():
    """Packed fp32 vector instructions beside fp32 MFMAs are corrupted by another wave's bf16 MFMAs on MI355X (profiles/
    NOTEBOOK_r05.md section 3; tests/test_gpu_stream_hazards.py): the build keeps the compiler from packing scalar math
    (-fno-slp-vectorize) and the sources do not ask for packed math outside narrow.hip (no MFMAs, never seen perturbed)."""
    from sketchyscenecolorization_amd import build
    assert build.NO_PACKED_FP32 == {'narrow.hip': []}
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith(('.hip', '.h')) and f != 'narrow.hip':
            txt = open(os.path.join(build.CSRC, f)).read()
            assert '__builtin_elementwise_fma' not in txt and '__builtin_elementwise_max' not in txt, f


# ---------------------------------------------------------------------------
# every entry point has a kernel-level GPU test
# ---------------------------------------------------------------------------
WHOLE_NETWORK_TESTS = {'test_gpu_pix2pix', 'test_gpu_mru', 'test_gpu_residual', 'test_gpu_fullsize', 'test_gpu_cli',
                       'test_gpu_checkpoint', 'test_gpu_two_ranks'}
# Entry points that launch nothing or only query / configure: the only ones that may go without a kernel test.  No arithmetic
# kernel may be listed here.
NOT_KERNEL_TESTED = {
    'ssc_version': 'host only: the ABI version (test_library_exports_every_declared_symbol)',
    'ssc_build_hash': 'host only: the source hash of the binary (test_stale_binary_is_refused)',
    'ssc_device_info': 'host only: device properties query',
    'ssc_timestamp': 'profiling aid: stores the wall clock, no arithmetic',
    'ssc_bf16_prepare': 'allocates per-device constants, launches nothing',
    'ssc_conv_forward_kernel_name': 'host only: name of the tile configuration',
    'ssc_conv_forward_plan': 'host only: the launch plan of a descriptor',
    'ssc_conv_rider_plan': 'host only: which path a conv with a reduction on its epilogue takes',
    'ssc_conv_fewchan_supported': 'host only: dispatch predicate',
    'ssc_conv_narrow_supported': 'host only: dispatch predicate',
    'ssc_conv_wgrad128_supported': 'host only: dispatch predicate',
    'ssc_conv_wgrad128_plan': 'host only: the launch plan of the 128 x 128 filter-gradient kernels',
    'ssc_conv_bf_plan': 'host only: the launch plan of the bf16x6 forward conv kernels',
    'ssc_conv_stream_plan': 'host only: the launch plan of the streaming forward conv kernels',
    'ssc_head1_forward_supported': 'host only: dispatch predicate',
}
# Arithmetic entry points that ssc_conv_forward / ssc_conv_wgrad call themselves when the launch qualifies (the header says
# "dispatches to it when _supported"): entry -> (the dispatcher, the kernel test that drives that path).  The dispatcher must be
# covered and the test must exist; nothing else may be listed here.
REACHED_THROUGH_THE_DISPATCHER = {
    'ssc_conv_narrow_forward': ('ssc_conv_forward', 'test_conv_forward_padded_channels_and_cout1'),
    'ssc_conv_wgrad128': ('ssc_conv_wgrad', 'test_wgrad128_conv'),
    'ssc_head1_forward': ('ssc_conv_forward', 'test_head1_patch_head'),
    'ssc_head1_dgrad': ('ssc_conv_forward', 'test_head1_patch_head'),
    'ssc_head1_wgrad': ('ssc_conv_wgrad', 'test_head1_patch_head'),
}
GENERIC_WRAPPERS = {'call', 'lib', 'check', '_declare', 'build_hash', 'check_build_hash'}     # name no entry point of their own


def _wrapper_map():
    """hip.<function> -> the ssc_* entry points it reaches (directly or through other functions of hip.py)."""
    import ast
    path = os.path.join(ROOT, 'sketchyscenecolorization_amd', 'hip.py')
    src = open(path).read()
    tree = ast.parse(src)
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    direct, calls = {}, {}
    for name, node in funcs.items():
        seg = ast.get_source_segment(src, node)
        direct[name] = set(re.findall(r'\bssc_\w+', seg))
        calls[name] = {c.func.id for c in ast.walk(node) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)
                       and c.func.id in funcs and c.func.id not in GENERIC_WRAPPERS}
    changed = True
    while changed:
        changed = False
        for name in funcs:
            for c in calls[name]:
                if not direct[c] <= direct[name]:
                    direct[name] |= direct[c]
                    changed = True
    return {k: v for k, v in direct.items() if k not in GENERIC_WRAPPERS and not k.startswith('_')}


def _uncovered(test_text):
    wrappers = _wrapper_map()
    used = {w for w in wrappers if re.search(r'\.%s\(' % re.escape(w), test_text)}
    reached = set().union(*[wrappers[w] for w in used]) if used else set()
    named = {n for n in _declared() if n in reached or re.search(r'\b%s\b' % n, test_text)}
    for n, (dispatcher, test) in REACHED_THROUGH_THE_DISPATCHER.items():
        if dispatcher in named and re.search(r'\bdef %s\(' % test, test_text):
            named.add(n)
    return sorted(n for n in _declared() if n not in NOT_KERNEL_TESTED and n not in named)


def _kernel_test_files():
    tdir = os.path.join(ROOT, 'tests')
    return sorted(os.path.join(tdir, f) for f in os.listdir(tdir)
                  if f.startswith('test_gpu_') and f.endswith('.py') and f[:-3] not in WHOLE_NETWORK_TESTS)


def test_every_entry_point_has_a_kernel_level_gpu_test():
    """Every ssc_* entry point of the header is named -- itself, or the hip.<wrapper> that reaches it -- in a tests/test_gpu_*.py
    file other than the whole-network ones, or sits in NOT_KERNEL_TESTED with a reason (query / no-launch entry points only,
    at most 25).  A new arithmetic entry point without a kernel test fails here, on any machine."""
    assert len(NOT_KERNEL_TESTED) <= 25
    assert set(NOT_KERNEL_TESTED) <= _declared(), set(NOT_KERNEL_TESTED) - _declared()
    for n in NOT_KERNEL_TESTED:
        assert n in ('ssc_version', 'ssc_build_hash', 'ssc_device_info', 'ssc_timestamp', 'ssc_sk_configure', 'ssc_bf16_prepare') \
            or n.endswith(('_supported', '_kernel_name', '_plan')), n + ': only query / no-launch entry points may be listed'
    assert set(REACHED_THROUGH_THE_DISPATCHER) <= _declared() and len(REACHED_THROUGH_THE_DISPATCHER) <= 5
    text = ''.join(open(f).read() for f in _kernel_test_files())
    missing = _uncovered(text)
    assert not missing, 'entry points without a kernel-level GPU test: %s' % missing


def test_the_coverage_check_notices_a_removed_kernel_test():
    """Without the file that tests the loss kernels the check names them."""
    text = ''.join(open(f).read() for f in _kernel_test_files() if not f.endswith('test_gpu_small_kernels.py'))
    missing = _uncovered(text)
    assert 'ssc_adam_tf' in missing and 'ssc_sn_backward_any' in missing and 'ssc_softplus_loss' in missing, missing
