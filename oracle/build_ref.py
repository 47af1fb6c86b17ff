"""Build oracle/_ref/ from /root/reference where the sources lie (nothing copied):

  * ref_primitives: the reference's header-inline primitives, through the harness
    oracle/ref_primitives.pyx;
  * seekmer/_common, seekmer/_mapper, seekmer/_index_builder: the reference's own three
    Cython modules, compiled from their place into the package oracle/_ref/seekmer/ beside an
    empty __init__.py of our own.  They `import logbook` and `import tables`, which this
    image lacks; the two stand-ins under oracle/ref_stubs/ (own code, a few lines each)
    satisfy the imports.  Logging and HDF5 I/O are not on the computation path.

Only runs where /root/reference exists (this container).  Outputs go to oracle/_ref/ only,
which is git-ignored: nothing compiled from the reference is committed.  The pins that are
committed are the fixtures these builds wrote: tests/golden/primitives.json
(make_primitives_golden.py) and tests/golden/reference_mapper.npz, reference_builder.npz
(make_reference_recordings.py)."""
import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
OUT = os.path.join(HERE, '_ref')
REF_MODULES = ('_common', '_mapper', '_index_builder')


def _compile(src, c_file, so, extra_includes=()):
    # legacy_implicit_noexcept: the semantics of the Cython 0.28 the reference pins
    # (environment.yml:9); results do not depend on it.
    subprocess.check_call([sys.executable, '-m', 'cython', '-3', '-I', REF,
                           '-X', 'legacy_implicit_noexcept=True',
                           src, '-o', c_file], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    cmd = ['gcc', '-O2', '-fPIC', '-shared', '-w', '-I', sysconfig.get_paths()['include']]
    for inc in extra_includes:
        cmd += ['-I', inc]
    subprocess.check_call(cmd + [c_file, '-o', so])


def _fresh(so, src):
    return os.path.exists(so) and os.path.getmtime(so) >= os.path.getmtime(src)


def build_modules(force=False):
    """The reference's three .pyx modules -> oracle/_ref/seekmer/<name><EXT_SUFFIX>."""
    import numpy
    package = os.path.join(OUT, 'seekmer')
    os.makedirs(package, exist_ok=True)
    init = os.path.join(package, '__init__.py')
    if not os.path.exists(init):
        with open(init, 'w'):
            pass
    ext = sysconfig.get_config_var('EXT_SUFFIX')
    built = []
    for name in REF_MODULES:
        src = os.path.join(REF, 'seekmer', name + '.pyx')
        so = os.path.join(package, name + ext)
        if force or not _fresh(so, src):
            _compile(src, os.path.join(package, name + '.c'), so, [numpy.get_include()])
        built.append(so)
    return built


def available():
    """True where build_modules() has left all three modules."""
    ext = sysconfig.get_config_var('EXT_SUFFIX')
    return all(os.path.exists(os.path.join(OUT, 'seekmer', name + ext)) for name in REF_MODULES)


def build(force=False):
    if not os.path.isdir(os.path.join(REF, 'seekmer')):
        return None
    os.makedirs(OUT, exist_ok=True)
    ext = sysconfig.get_config_var('EXT_SUFFIX')
    so = os.path.join(OUT, 'ref_primitives' + ext)
    src = os.path.join(HERE, 'ref_primitives.pyx')
    if force or not _fresh(so, src):
        _compile(src, os.path.join(OUT, 'ref_primitives.c'), so)
    build_modules(force)
    return so


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
