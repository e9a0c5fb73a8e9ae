"""The reference's own C (oracle/_ref/libbwaref.so) as the tests see it: live where the reference build exists, replayed from a
recording of the same calls (tests/golden/ref_calls/<module>__<test>.npz) where it does not.

Every call is recorded as (method, digest of its arguments, result).  Replaying, a call must name the same method with arguments of
the same digest as the recording's call at that position, so a test whose inputs changed fails instead of being compared with
outputs of other inputs.  Live with a recording present, every result must equal the recorded one, so the recordings stay what
the reference computes.  BPSW_REF_RECORD=DIR writes the recordings of the tests that ran (live only) into DIR."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

RECORDINGS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls")


def recording_path(module: str, test: str, root: str = RECORDINGS) -> str:
    return os.path.join(root, f"{module}__{test}.npz")


def _digest(h, x):
    if isinstance(x, np.ndarray):
        h.update(b"nd" + str(x.dtype.descr).encode() + str(x.shape).encode())
        h.update(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, (bytes, bytearray)):
        h.update(b"by" + bytes(x))
    elif x is None or isinstance(x, (bool, int, float, str, np.integer, np.floating)):
        h.update(b"sc" + repr(x.item() if isinstance(x, (np.integer, np.floating)) else x).encode())
    elif isinstance(x, (list, tuple)):
        h.update(b"sq%d" % len(x))
        for v in x:
            _digest(h, v)
    elif isinstance(x, dict):
        h.update(b"di%d" % len(x))
        for k in sorted(x):
            h.update(str(k).encode())
            _digest(h, x[k])
    elif isinstance(x, C.Structure):
        h.update(b"st" + type(x).__name__.encode())
        for f in x._fields_:
            _digest(h, getattr(x, f[0]))
    elif isinstance(x, C.Array):
        _digest(h, list(x))
    elif hasattr(x, "__dict__"):
        h.update(b"ob" + type(x).__name__.encode())
        _digest(h, {k: v for k, v in vars(x).items() if not k.startswith("_") and not callable(v)})
    else:
        h.update(b"ty" + type(x).__name__.encode())


def digest(args, kwargs) -> str:
    h = hashlib.sha256()
    _digest(h, list(args))
    _digest(h, dict(kwargs))
    return h.hexdigest()[:32]


def _encode(x, blobs):
    """a result as a JSON-able tree whose arrays and byte strings point into `blobs` (one uint8 buffer in the end)"""
    if isinstance(x, np.ndarray):
        blobs.append(np.ascontiguousarray(x).tobytes())
        return {"nd": [x.dtype.descr if x.dtype.names else x.dtype.str, list(x.shape)]}
    if isinstance(x, (bytes, bytearray)):
        blobs.append(bytes(x))
        return {"by": len(x)}
    if isinstance(x, (np.integer, np.floating)):
        x = x.item()
    if x is None or isinstance(x, (bool, int, float, str)):
        return {"sc": x}
    if isinstance(x, (list, tuple)):
        return {"tu" if isinstance(x, tuple) else "li": [_encode(v, blobs) for v in x]}
    raise TypeError(f"cannot record a result of type {type(x).__name__}")


def _decode(t, blob, at):
    """the inverse of _encode; at = [offset into blob], advanced past what was read"""
    if "nd" in t or "by" in t:
        if "nd" in t:
            descr, shape = t["nd"]
            dt = np.dtype([tuple(f) for f in descr] if isinstance(descr, list) else descr)
            n = dt.itemsize * int(np.prod(shape, dtype=np.int64))
        else:
            n = t["by"]
        raw = blob[at[0]:at[0] + n].tobytes()
        at[0] += n
        return np.frombuffer(raw, dt).reshape(shape).copy() if "nd" in t else raw
    if "sc" in t:
        return t["sc"]
    vals = [_decode(v, blob, at) for v in t.get("tu", t.get("li"))]
    return tuple(vals) if "tu" in t else vals


def same(a, b) -> bool:
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes())
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.integer, np.floating)):
        a = a.item()
    if isinstance(b, (np.integer, np.floating)):
        b = b.item()
    return type(a) is type(b) and a == b


def load(path):
    z = np.load(path)
    calls = json.loads(z["calls"].tobytes().decode())
    blob, at, out = z["blob"], [0], []
    for method, dig, tree in calls:
        out.append((method, dig, _decode(tree, blob, at)))
    return out


def save(path, made):
    """made: RefCalls.made, [(method, digest, tree, bytes)]"""
    trees = [[method, dig, tree] for method, dig, tree, _ in made]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, calls=np.frombuffer(json.dumps(trees).encode(), np.uint8),
                        blob=np.frombuffer(b"".join(raw for *_, raw in made), np.uint8))


class RefCalls:
    """stands in for pyoracle.Ref: `live` (a pyoracle.Ref or None) answers when there, the recording `calls` (load) otherwise"""

    def __init__(self, live, calls, where):
        self._live, self._calls, self._where, self._n, self.made = live, calls, where, 0, []

    def __getattr__(self, method):
        if method.startswith("_"):
            raise AttributeError(method)

        def call(*args, **kwargs):
            dig = digest(args, kwargs)
            rec = None
            if self._calls is not None:
                assert self._n < len(self._calls), f"{self._where}: more reference calls than recorded ({len(self._calls)})"
                rec = self._calls[self._n]
                assert rec[0] == method and rec[1] == dig, \
                    f"{self._where}: call {self._n} is {method} on other inputs than recorded ({rec[0]}); re-record with the reference build"
            self._n += 1
            if self._live is None:
                return rec[2]
            got = getattr(self._live, method)(*args, **kwargs)
            if rec is not None:
                assert same(got, rec[2]), f"{self._where}: call {self._n - 1} ({method}) differs from the recording"
            blobs = []
            tree = _encode(got, blobs)              # (encoded now: a later call may reuse the buffers behind `got`)
            self.made.append((method, dig, tree, b"".join(blobs)))
            return got
        return call

    def finish(self):
        """at the end of a test that passed: every recorded call was made"""
        if self._calls is not None:
            assert self._n == len(self._calls), f"{self._where}: {self._n} reference calls made, {len(self._calls)} recorded"
