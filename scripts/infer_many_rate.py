"""What `seekmer_amd infer-many` buys: N samples of P read pairs each, written as FASTQ files, quantified
    (a) by N runs of `seekmer_amd infer`, each a fresh child process that loads and uploads the index again,
    (b) by one `infer-many` process whose small samples share launches in a sample set,
    (c) by one `infer-many` process with SKM_INFER_MANY_PER_SAMPLE=1 (a mapper per sample on the resident index),
with every sample's abundance.tsv compared byte for byte between the three.
    python3 scripts/infer_many_rate.py --samples 64 --pairs 20000 --genes 100
    python3 scripts/infer_many_rate.py --samples 64 --pairs 20000 --genes 20000 --cache /tmp/skm_idx.npz
Wall time of whole processes, as a user sees it (interpreter start, index load and upload, first-use costs, reading
the files, writing the outputs).  Making the index and the files happens before any clock starts.  Every step
that uses the GPU is a child process under a time limit of its own (`timeout -k 10 SECONDS ...`); the script stops
at the first step that fails and starts nothing again.
"""
import argparse
import os
import pathlib
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--samples', type=int, default=64)
ap.add_argument('--pairs', type=int, default=20000)
ap.add_argument('--genes', type=int, default=100)
ap.add_argument('--read-len', type=int, default=75)
ap.add_argument('--jobs', type=int, default=4)
ap.add_argument('--bootstrap', type=int, default=0)
ap.add_argument('--cache', default='', help='keep the index in this file between invocations')
ap.add_argument('--step-limit', type=int, default=300, help='seconds one child process may take')
ap.add_argument('--work', default='', help='folder for the files (default: a temporary one)')
args = ap.parse_args()


def step(name, arguments, env=None):
    """One child process under its own time limit; the first failure ends the script."""
    t0 = time.perf_counter()
    done = subprocess.run(['timeout', '-k', '10', str(args.step_limit), sys.executable, '-m', 'seekmer_amd'] + arguments,
                          cwd=ROOT, env=dict(os.environ, **(env or {})), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if done.returncode != 0:
        sys.stderr.write(done.stderr.decode(errors='replace')[-4000:])
        sys.exit('%s ended with status %d after %.1f s: nothing more is started' % (name, done.returncode, dt))
    return dt


def main():
    from seekmer_amd import common, index_builder, synth     # (host code only: this process never opens the GPU)
    work = pathlib.Path(args.work or tempfile.mkdtemp(prefix='skm_infer_many_'))
    work.mkdir(parents=True, exist_ok=True)
    ids, pool, tx_offsets = synth.transcriptome(1, args.genes)
    index_path = pathlib.Path(args.cache) if args.cache else work / 'index.npz'
    if not index_path.exists():
        index_builder.build_pooled(ids, pool, tx_offsets).save(index_path)
    files = []
    for sample in range(args.samples):
        bases, _ = synth.reads(100 + sample % 2, pool, tx_offsets, sample * args.pairs, args.pairs, args.read_len, True)
        mates = [work / ('s%03d_%d.fastq' % (sample, mate)) for mate in (1, 2)]
        synth.write_fastq(bases, args.pairs, args.read_len, True, *mates)
        files += mates
    print('%d samples x %d pairs of 2 x %d bases on %d transcripts; index of %.0f MiB' %
          (args.samples, args.pairs, args.read_len, len(ids), index_path.stat().st_size / 2 ** 20), flush=True)
    extra = ['-b', str(args.bootstrap), '--seed', '1'] if args.bootstrap else []
    alone = []
    for sample in range(args.samples):
        alone.append(step('infer of sample %d' % sample,
                          ['infer', str(index_path), str(work / 'alone' / ('s%03d_1' % sample)),
                           *map(str, files[2 * sample:2 * sample + 2])] + extra))
    print('infer, a process per sample: %.2f s in all; per sample %.2f s (fastest %.2f, slowest %.2f)'
          % (sum(alone), sum(alone) / len(alone), min(alone), max(alone)), flush=True)
    many = [str(index_path), None, *map(str, files), '-j', str(args.jobs)] + extra
    many[1] = str(work / 'many_set')
    in_set = step('infer-many', ['infer-many'] + many, env={'SKM_INFER_MANY_PER_SAMPLE': '0'})
    print('infer-many, sample set:       %.2f s (%.1f x)' % (in_set, sum(alone) / in_set), flush=True)
    many[1] = str(work / 'many_one_by_one')
    one_by_one = step('infer-many, a mapper per sample', ['infer-many'] + many, env={'SKM_INFER_MANY_PER_SAMPLE': '1'})
    print('infer-many, mapper per sample: %.2f s (%.1f x)' % (one_by_one, sum(alone) / one_by_one), flush=True)
    for sample in range(args.samples):
        name = 's%03d_1' % sample
        want = (work / 'alone' / name / 'abundance.tsv').read_bytes()
        for form in ('many_set', 'many_one_by_one'):
            assert (work / form / name / 'abundance.tsv').read_bytes() == want, '%s of %s differs from infer' % (name, form)
    print('all %d abundance.tsv agree byte for byte between the three forms' % args.samples, flush=True)


if __name__ == '__main__':
    main()
