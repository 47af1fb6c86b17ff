"""The C-ABI libraries load on a machine without a GPU and export every symbol
include/seekmer_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

from conftest import ROOT


def _declared_symbols():
    with open(os.path.join(ROOT, 'include', 'seekmer_hip.h')) as f:
        text = f.read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(skm_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_expected_families():
    names = _declared_symbols()
    for family in ('skm_index_create', 'skm_mapper_map_batch', 'skm_mapper_export', 'skm_quant_em',
                   'skm_quant_bootstrap', 'skm_effective_lengths', 'skm_build_index',
                   'skm_fastq_next', 'skm_synth_reads', 'skm_comm_unique_id'):
        assert family in names


def test_every_declared_symbol_is_exported_and_bound(native_libs):
    hip = ctypes.CDLL(native_libs.HIP_LIB_PATH)
    host = ctypes.CDLL(native_libs.HOST_LIB_PATH)
    bound = set(native_libs.HIP_SYMBOLS) | set(native_libs.HOST_SYMBOLS)
    for name in _declared_symbols():
        assert hasattr(hip, name) or hasattr(host, name), name + ' is declared but not exported'
        assert name in bound, name + ' is declared but not bound in seekmer_amd/_native.py'
    for name in bound:
        assert name in _declared_symbols(), name + ' is bound but not declared in the header'
    native_libs.hip()
    native_libs.host()


def _defined_dynamic_symbols(path):
    """`nm -D --defined-only` of a shared library: binutils' nm, or else the llvm-nm that stands beside hipcc."""
    import shutil
    import subprocess
    import pytest
    hipcc = shutil.which(os.environ.get('HIPCC', 'hipcc')) or '/opt/rocm/bin/hipcc'
    beside = os.path.dirname(os.path.realpath(hipcc))
    tools = [shutil.which('nm'), os.path.join(beside, 'llvm-nm'), os.path.join(beside, '..', 'lib', 'llvm', 'bin', 'llvm-nm'),
             os.path.join(beside, '..', 'llvm', 'bin', 'llvm-nm')]
    tools = [t for t in tools if t and os.path.exists(t)]
    if not tools:
        pytest.skip('neither nm nor llvm-nm')
    lines = subprocess.check_output([tools[0], '-D', '--defined-only', path], text=True).splitlines()
    return [line.split()[-1].split('@')[0] for line in lines if line.strip()]


def test_the_gpu_library_exports_the_c_abi_and_nothing_of_the_glue(native_libs):
    """The glue's units share their helpers through the hidden namespace skm::abi: none of them is a dynamic symbol,
    and the library's skm_* symbols are exactly the header's declarations that the host library does not export."""
    hip = _defined_dynamic_symbols(native_libs.HIP_LIB_PATH)
    host = _defined_dynamic_symbols(native_libs.HOST_LIB_PATH)
    assert hip and host
    assert [name for name in hip if '3skm3abi' in name] == []
    exported = sorted(name for name in hip if name.startswith('skm_'))
    assert len(exported) == len(set(exported))
    assert exported == sorted(set(_declared_symbols()) - set(host))


def test_no_gpu_fails_loudly(native_libs):
    """Without a GPU every device entry point must fail, never fall back."""
    import numpy as np
    import pytest
    if native_libs.device_count() > 0:
        pytest.skip('a GPU is present')
    n = ctypes.c_int(-1)
    assert native_libs.hip().skm_device_count(ctypes.byref(n)) == native_libs.SKM_ERR_NO_DEVICE
    assert b'no HIP device' in native_libs.hip().skm_last_error()
    fld = np.zeros(2000, dtype=np.int64)
    length = np.ones(4)
    out = np.zeros(4)
    code = native_libs.hip().skm_effective_lengths(
        0, native_libs.ptr(fld, native_libs.c_i64p), native_libs.ptr(length, native_libs.c_f64p), 4,
        native_libs.ptr(out, native_libs.c_f64p))
    assert code == native_libs.SKM_ERR_NO_DEVICE


def test_product_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/."""
    pkg = os.path.join(ROOT, 'seekmer_amd')
    for base, _, files in os.walk(pkg):
        for name in files:
            if name.endswith(('.py', '.cpp', '.hip', '.h')):
                with open(os.path.join(base, name), errors='replace') as f:
                    text = f.read()
                assert 'skmo_' not in text, name
                assert 'import oracle' not in text and 'from oracle' not in text, name
                assert 'libskm_oracle' not in text, name


def test_the_production_map_kernel_does_not_spill(native_libs):
    """map_units_kernel<false, true> runs at 128 VGPRs (4 waves per SIMD) WITHOUT scratch: 7 spilled registers were
    3 GB of HBM writes per 10 M pairs in the counters of round 4 (WRITE_SIZE x 7), caused by moving one branch of the
    action switch.  The build keeps the compiler's resource remarks beside the object."""
    import re
    import subprocess
    remarks = os.path.join(ROOT, 'seekmer_amd', 'csrc', 'build', 'skm_map.remarks')
    if not os.path.exists(remarks):
        subprocess.check_call(['touch', os.path.join(ROOT, 'seekmer_amd', 'csrc', 'skm_map.hip')])
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'seekmer_amd', 'csrc')], stdout=subprocess.DEVNULL)
    text = open(remarks).read()
    blocks = text.split('Function Name: ')
    mine = [b for b in blocks if b.startswith('_ZN3skm16map_units_kernelILb0ELb1EEE')]
    assert len(mine) == 1
    scratch = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', mine[0]).group(1))
    vgprs = int(re.search(r' VGPRs: (\d+)', mine[0]).group(1))
    spilled = int(re.search(r'VGPRs Spill: (\d+)', mine[0]).group(1))
    assert scratch == 0 and spilled == 0 and vgprs <= 128, (scratch, spilled, vgprs)
