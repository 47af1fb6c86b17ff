"""Record what the COMPILED REFERENCE computes on the cases of tests/reference_cases.py:

    tests/golden/reference_mapper.npz    per mapper case: units, paired flag, SHA-256 of the reads,
                                         per-unit target counts, flat unsigned ids (as _get_ids
                                         returns them), the 2 000-bin fragment-length histogram
    tests/golden/reference_builder.npz   per builder case: sizes of the four arrays, slot 0 occupied
                                         or not and its row, occupied-slot count, SHA-256 digests of
                                         the arrays (reference_cases.index_digests); contig table,
                                         pooled bases and targets whole where slot 0 is occupied or
                                         the case has at most 50 transcripts; for the latter the
                                         k-mer table too, occupied slots only
                                         (reference_cases.pack_table / unpack_table)

Runs on the build machine only, where oracle/build_ref.py has compiled the reference's _common,
_mapper and _index_builder into oracle/_ref/seekmer/, and as a process of its own: the stand-ins
for logbook and tables (oracle/ref_stubs) must never enter a pytest process.

    python oracle/build_ref.py && python tests/golden/make_reference_recordings.py [--check]

--check records again in memory and compares with the committed files (exit status 1 on any
difference): the staleness test of tests/test_reference_recordings.py.
"""
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, 'oracle', 'ref_stubs'), os.path.join(ROOT, 'oracle', '_ref'),
                os.path.join(ROOT, 'tests'), ROOT]

import reference_cases as cases                                     # noqa: E402
from oracle import oracle as O                                      # noqa: E402  (file readers only)
from seekmer._common import KMerIndex                               # noqa: E402
from seekmer._index_builder import ContigAssembler                  # noqa: E402
from seekmer._mapper import ReadMapper                              # noqa: E402

MAPPER_FILE = os.path.join(HERE, 'reference_mapper.npz')
BUILDER_FILE = os.path.join(HERE, 'reference_builder.npz')


class _Result:
    """What ReadMapper.__call__ needs of a MapResult (seekmer/_mapper.pyx:100-105)."""

    def __init__(self):
        self.lock = threading.Lock()
        self.tuples = []
        self.fld = np.zeros(2000, dtype=np.int64)

    def update(self, read_names, ids):
        self.tuples.extend(ids)

    def merge_fragment_lengths(self, counts):
        self.fld += counts


def _smallest_unsigned(values):
    top = int(values.max()) if values.size else 0
    return values.astype('<u2' if top < 1 << 16 else '<u4')


def record_mapper(seqs, pairs21):
    out = {}
    kmers, contigs, sequences, targets = ContigAssembler().assemble(seqs)
    assert kmers['kmer'][0] == np.uint64(cases.INVALID_KMER)       # slot 0 empty: see SURVEY.md
    index = KMerIndex(kmers, contigs, sequences, targets, None, None)
    names = []
    for name, paired, reads in cases.mapper_cases(seqs, pairs21):
        n_units = len(reads) // 2 if paired else len(reads)
        result = _Result()
        ReadMapper(index, result)(iter([(n_units, [b''] * n_units, reads)]))
        assert len(result.tuples) == n_units
        flat = np.array([i for t in result.tuples for i in t], dtype=np.int64)
        assert flat.size == 0 or flat.min() >= 0
        out[name + '/units'] = np.int64(n_units)
        out[name + '/paired'] = np.bool_(paired)
        out[name + '/sha256'] = np.str_(cases.reads_digest(reads))
        out[name + '/counts'] = _smallest_unsigned(np.array([len(t) for t in result.tuples], dtype=np.int64))
        out[name + '/ids'] = _smallest_unsigned(flat)
        out[name + '/fld'] = result.fld.astype('<i4')
        names.append(name)
    out['cases'] = np.array(names)
    return out


def record_builder(seqs, extra_seqs):
    out = {}
    names = []
    for name, transcripts in cases.builder_cases(seqs, extra_seqs):
        kmers, contigs, sequences, targets = ContigAssembler().assemble(transcripts)
        occupied = kmers['kmer'] != np.uint64(cases.INVALID_KMER)
        out[name + '/transcripts'] = np.int64(len(transcripts))
        out[name + '/sizes'] = np.array([kmers.size, contigs.size, sequences.size, targets.size], dtype='<i8')
        out[name + '/slot0_occupied'] = np.bool_(occupied[0])
        out[name + '/slot0_row'] = np.array([kmers['kmer'][0].view('<i8'), kmers['entry'][0],
                                             kmers['offset'][0]], dtype='<i8')
        out[name + '/occupied'] = np.int64(occupied.sum())
        for key, value in cases.index_digests(kmers, contigs, sequences, targets).items():
            out[name + '/sha256/' + key] = np.str_(value)
        small = len(transcripts) <= cases.SPARSE_LIMIT
        if small or occupied[0]:
            out[name + '/contigs'] = np.stack([np.asarray(contigs[f]).astype('<u8').view('<i8')
                                               for f in contigs.dtype.names], axis=1)
            out[name + '/sequences'] = np.frombuffer(np.asarray(sequences).tobytes(), dtype=np.uint8)
            out[name + '/targets'] = np.stack([targets['entry'], targets['offset']], axis=1).astype('<i4')
        if small:
            slots = np.flatnonzero(occupied)
            packed = cases.pack_table(slots, kmers['kmer'][slots], kmers['entry'][slots],
                                      kmers['offset'][slots])
            for key, value in packed.items():
                out[name + '/table/' + key] = value
        names.append(name)
    out['cases'] = np.array(names)
    return out


def _differences(path, fresh):
    with np.load(path) as stored:
        keys = set(stored.files)
        bad = sorted(keys ^ set(fresh))
        for key in sorted(keys & set(fresh)):
            a, b = stored[key], np.asarray(fresh[key])
            if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
                bad.append(key)
    return bad


def main(argv):
    _, seqs = O.read_fasta(os.path.join(HERE, 'human.cdna.21.fa.bz2'))
    _, extra = O.read_fasta(os.path.join(HERE, 'human.cdna.21.with_extra.fa.gz'))
    pairs21 = O.read_fastq_pairs(os.path.join(HERE, '20_1.fastq'), os.path.join(HERE, '20_2.fastq'))
    recorded = ((MAPPER_FILE, record_mapper(seqs, pairs21)), (BUILDER_FILE, record_builder(seqs, extra)))
    if '--check' in argv:
        status = 0
        for path, fresh in recorded:
            bad = _differences(path, fresh)
            print(os.path.basename(path), 'differs in %s' % bad if bad else 'is what the reference gives')
            status |= bool(bad)
        return status
    for path, fresh in recorded:
        np.savez_compressed(path, **fresh)
        print('wrote', os.path.basename(path), os.path.getsize(path), 'bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
