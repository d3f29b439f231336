"""What the pinned fault tables share (test_gpu_model_errors.py, test_gpu_context_errors.py): sentinel-filled outputs that know whether a call left them alone, the golden's format
(one call per line: [name, code, error, untouched]), its recording and the comparison against it."""
import ctypes as C
import json

import numpy as np

FIELDS = ("name", "code", "error", "untouched")
SENTINEL = -12345.0


class Outs:
    """the outputs of one call, sentinel-filled, and whether the call left them alone"""

    def __init__(self):
        self.kept = []

    def _keep(self, x, raw):
        self.kept.append((x, raw))
        return x

    def arr(self, shape, dtype=np.float32):
        a = np.full(shape, 0xA5 if dtype == np.uint8 else SENTINEL, dtype)
        return self._keep(a, a.tobytes())

    def pose(self, values=None, n=1):
        a = np.zeros(6 * n) if values is None else np.array(values, np.float64).reshape(-1)
        return self._keep(a, a.tobytes())

    def stats(self, struct, n=1):
        s = (struct * n)()
        C.memset(s, 0xA5, C.sizeof(s))
        return self._keep(s, bytes(s))

    def i64(self):
        return C.byref(self._keep(C.c_int64(-7), bytes(C.c_int64(-7))))

    def untouched(self):
        return all((x.tobytes() if isinstance(x, np.ndarray) else bytes(x)) == raw for x, raw in self.kept)


def compare_with_golden(path, got):
    with open(path) as fh:
        want = [dict(zip(FIELDS, row)) for row in json.load(fh)]
    assert [r["name"] for r in got] == [r["name"] for r in want]
    wrong = [(w, r) for w, r in zip(want, got) if w != r]
    for w, r in wrong:
        print(f"  {w['name']}:\n    recorded {w}\n    now      {r}")
    assert not wrong, f"{len(wrong)} of {len(want)} calls differ from the recorded fault table"
    assert all(r["code"] != 0 and r["error"] and r["untouched"] for r in want)      # the record itself: every call refused, with a text, nothing written


def record_golden(path, rows, lib_path):
    """writes the table; the exit status says whether every call was a refused one that left its outputs alone"""
    bad = [r for r in rows if r["code"] == 0 or not r["error"] or not r["untouched"]]
    for r in bad:
        print("not a refused call that leaves its outputs alone:", r)
    with open(path, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps([r[k] for k in FIELDS]) for r in rows) + "\n]\n")
    print(f"{len(rows)} calls recorded to {path} from {lib_path}; {len(bad)} of them unexpected")
    return 1 if bad else 0
