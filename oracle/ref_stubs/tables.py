"""Stand-in for `tables` (PyTables), for the compiled reference modules under oracle/_ref/
only (oracle/build_ref.py).  The reference touches it in KMerIndex.save/load alone, which
nothing here calls: an empty module is enough for the import to succeed."""
