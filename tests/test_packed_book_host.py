"""The packed pieces' book (seekmer_amd/csrc/skm_packed_book.h), the host arithmetic that decides which packed reads
meet as mates, on a CPU: scripts/micro/packed_book_asan.cpp drives it through random inserts, replacements, cuts, runs
and drops against a per-unit model, as a program of its own under AddressSanitizer + UBSan (no GPU, no Python in the
process, nothing preloaded)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, 'seekmer_amd', 'csrc')
PROGRAM = os.path.join(ROOT, 'scripts', 'micro', 'packed_book_asan.cpp')


def test_the_header_needs_no_hip_and_nothing_of_the_glue(tmp_path):
    """g++ alone compiles it, with no include path at all."""
    source = tmp_path / 'only_the_book.cpp'
    source.write_text('#include "%s"\nint main() { return skm::abi::PackedBook().empty() ? 0 : 1; }\n'
                      % os.path.join(CSRC, 'skm_packed_book.h'))
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', str(source)])
    with open(os.path.join(CSRC, 'skm_packed_book.h')) as f:
        includes = [line.split()[1] for line in f if line.startswith('#include')]
    assert includes and all(name.startswith('<') and 'hip' not in name for name in includes), includes


def test_book_matches_a_per_unit_model_under_asan_ubsan(tmp_path):
    binary = tmp_path / 'packed_book_asan'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-static-libasan', '-static-libubsan', '-I', CSRC, PROGRAM, '-o', str(binary)])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    proc = subprocess.run([str(binary)], env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    assert proc.stdout.strip().endswith('ok')
    assert 'runtime error' not in proc.stderr and 'AddressSanitizer' not in proc.stderr, proc.stderr[-3000:]
