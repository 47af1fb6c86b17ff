"""Stand-in for `logbook`, for the compiled reference modules under oracle/_ref/ only
(oracle/build_ref.py).  The reference logs progress and nothing else through it; a Logger
that swallows every call keeps logging off the computation path.  Only the recorder
(tests/golden/make_reference_recordings.py) puts this directory on its path, in a process
of its own."""


class Logger:
    def __init__(self, *args, **kwargs):
        pass

    def __getattr__(self, name):
        return lambda *args, **kwargs: None
