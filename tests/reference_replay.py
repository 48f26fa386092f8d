"""The compiled reference's results, for checkouts where oracle/_ref cannot be built.

oracle/_ref is compiled from a checkout of the reference project, which only some build hosts have.  Where it is
missing, the `reference` fixture is a Replay: its calls run the C restatement (oracle/gs_oracle.c), and each test folds
every call it makes and that call's result, in call order, into one digest.  When the test ends, that digest must equal
the one the compiled reference produced for the same test (tests/golden/reference_digests.json), so a test still
compares against what the reference computed.  The few calls the restatement cannot make (a FAST score map of another
size than the image, which the reference addresses through gs_get / gs_set) return the reference's own result, stored
whole (tests/golden/reference_results.pkl.gz).  Only the default, derandomised examples of the property tests are
recorded.

Recording: GS_RECORD_REFERENCE=1 where oracle/_ref exists.  The fixture then wraps the compiled reference, runs the
restatement beside it, and merges the digests into the golden files at the end of the session; a test on which the two
disagree anywhere is recorded as such, and replaying it fails.
"""
import gzip
import hashlib
import json
import os
import pickle

import numpy as np

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")
VALUES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_results.pkl.gz")
MISMATCH = "restatement differs from the reference"


def _restatement_cannot(name, args, kwargs):
    """oracle/gs_oracle.c's FAST writes a score map of the image's size"""
    sm = kwargs.get("scoremap")
    return name == "fast" and sm is not None and sm.shape != np.shape(args[0])


def _canon(h, v):
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        h.update(("nd%r%r" % (a.dtype.descr, a.shape)).encode())
        h.update(a.tobytes())
    elif isinstance(v, (list, tuple)):
        h.update(b"seq%d" % len(v))
        for x in v:
            _canon(h, x)
    elif isinstance(v, dict):
        h.update(b"map%d" % len(v))
        for k in sorted(v):
            _canon(h, k)
            _canon(h, v[k])
    elif isinstance(v, np.generic):
        h.update(("%s:%r" % (v.dtype.str, v.item())).encode())
    elif v is None or isinstance(v, (bool, int, float, str)):
        h.update(("%s:%r" % (type(v).__name__, v)).encode())
    elif hasattr(v, "stage_threshold"):  # grayskull_amd.cascade.Cascade: its window and tables
        _canon(h, {k: x for k, x in vars(v).items() if not k.startswith("_")})
    else:
        raise TypeError("no canonical form for %r" % type(v))


def digest(*values):
    h = hashlib.sha1()
    for v in values:
        _canon(h, v)
    return h.hexdigest()[:20]


def _load():
    digests, values = {}, {}
    if os.path.exists(DIGESTS):
        with open(DIGESTS) as f:
            digests = json.load(f)
    if os.path.exists(VALUES):
        with gzip.open(VALUES, "rb") as f:
            values = pickle.load(f)
    return digests, values


class _Wrapper:
    def __init__(self, kind, lib):
        self.kind, self._lib = kind, lib
        self._test, self._chain = None, None

    def begin(self, test):
        self._test, self._chain = test, hashlib.sha1()

    def _fold(self, key, result):
        if self._chain is not None:
            self._chain.update((key + digest(result)).encode())

    def __getattr__(self, name):
        attr = getattr(self._lib, name)
        if not callable(attr) or name.startswith("_") or name in ("synth", "fnv1a"):  # the static helpers are not results
            return attr

        def call(*args, **kwargs):
            key = digest(self.kind, name, list(args), kwargs)
            out = self._call(key, name, args, kwargs)
            self._fold(key, out)
            return out
        return call


class Replay(_Wrapper):
    """the restatement; end() checks the test's calls and results against the reference's recorded digest"""
    def __init__(self, kind, port):
        super().__init__(kind, port)
        self._want, self._values = _load()

    def _call(self, key, name, args, kwargs):
        if key in self._values:
            return pickle.loads(self._values[key])  # a fresh copy: callers may write into what they get
        if _restatement_cannot(name, args, kwargs):
            raise AssertionError("no recorded result of the %s for this call: re-record with GS_RECORD_REFERENCE=1" % self.kind)
        return getattr(self._lib, name)(*args, **kwargs)

    def end(self):
        want, got = self._want.get(self._test), self._chain.hexdigest()[:20]
        test, self._test, self._chain = self._test, None, None
        assert want is not None, "no recorded %s results for %s: re-record %s with GS_RECORD_REFERENCE=1 where oracle/_ref " \
                                 "exists" % (self.kind, test, os.path.relpath(DIGESTS))
        assert want != MISMATCH and got == want, "%s: the C restatement's results differ from the recorded %s results" \
                                                 % (test, self.kind)


class Recorder(_Wrapper):
    """the compiled reference itself; records each test's digest, and whether the restatement agrees on every call"""
    def __init__(self, kind, ref, port):
        super().__init__(kind, ref)
        self._restatement, self._seen, self._kept, self._agree = port, {}, {}, True

    def begin(self, test):
        super().begin(test)
        self._agree = True

    def _call(self, key, name, args, kwargs):
        def cp(v):
            return v.copy() if isinstance(v, np.ndarray) else v
        args0, kwargs0 = [cp(v) for v in args], {k: cp(v) for k, v in kwargs.items()}  # as they were before the call
        ref = getattr(self._lib, name)(*args, **kwargs)
        if self._test is None:
            return ref
        if _restatement_cannot(name, args, kwargs):
            self._kept[key] = pickle.dumps(ref, protocol=4)
        else:
            self._agree &= digest(getattr(self._restatement, name)(*args0, **kwargs0)) == digest(ref)
        return ref

    def end(self):
        self._seen[self._test] = self._chain.hexdigest()[:20] if self._agree else MISMATCH
        self._test, self._chain = None, None

    def save(self):
        digests, values = _load()
        digests.update(self._seen)
        values.update(self._kept)
        with open(DIGESTS, "w") as f:
            json.dump(dict(sorted(digests.items())), f, indent=0)
            f.write("\n")
        with gzip.GzipFile(VALUES, "wb", mtime=0) as f:
            pickle.dump(dict(sorted(values.items())), f, protocol=4)
        return len(self._seen), sum(v == MISMATCH for v in self._seen.values())
