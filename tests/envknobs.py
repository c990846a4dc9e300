"""Helper shared by the test files that run the same work under different SPDP_* knobs (the library reads them
per call): sets environment variables for the duration of a `with` block and puts the old values back."""
import os


class Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
