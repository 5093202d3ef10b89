"""Helpers shared by the parity tests."""
import numpy as np

# what the tolerance-based tests actually measured (excluded shares, worst errors): printed by conftest's terminal summary
PARITY_NOTES = []


def parity_note(line):
    PARITY_NOTES.append(str(line))


# one record per compared gradient array: which criterion decided it, measured error next to the tolerance
# (conftest writes them to gpurun_out/parity_rows.jsonl; tools/parity_table.py turns them into the table of DESIGN.md 3)
PARITY_ROWS = []


def parity_row(**row):
    PARITY_ROWS.append(row)


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def to_np(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


from oracle.parity import dilate  # noqa: E402,F401  (shared with __graft_entry__.smoke())


def rel_err(a, b):
    """max |a-b| relative to the largest magnitude of the reference b."""
    b = np.asarray(b, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-30)
    return float(np.abs(a - b).max() / scale)


def assert_close_masked(got, want, tol, knife=None, what=""):
    """|got-want| <= tol * max|want| everywhere except at knife-edge positions (where the
    reference's strict `-1 < x < 1` test, models/transform.py:129, sits within rounding of
    the decision boundary and a 1-ulp difference legitimately flips a pixel to/from zero)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    scale = max(float(np.abs(want).max()), 1e-30)
    bad = np.abs(got - want) > tol * scale
    if knife is not None:
        bad &= ~np.broadcast_to(knife, bad.shape)
    assert not bad.any(), "%s: %d / %d elements off by more than %g (max rel err %g)" % (
        what, int(bad.sum()), bad.size, tol, float((np.abs(got - want) * ~np.broadcast_to(
            knife if knife is not None else np.zeros(1, bool), bad.shape)).max() / scale))


# ---------------------------------------------------------------------------------------------------------------------------
# Guarded placement of device buffers (tests/test_buffer_contracts_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FA5A5A5          # as float32: a NaN (exponent all ones, mantissa 0x25a5a5); as bytes nothing a kernel computes
GUARD_MIN_BYTES = 4096


class Arena:
    """ONE device allocation filled with SENTINEL words, from which named buffers are carved.

    specs: list of (name, shape, residue) -- a float32 array of that shape whose first byte lies at `residue` (0, 4, 8, 12) mod 16
           -- or (name, nbytes, "ws"): `nbytes` bytes of scratch that start on a 256-byte boundary and end exactly there.
    Every buffer has at least max(4 KiB, two rows of the widest array: 2 * 4 * row_floats bytes) of sentinel on both sides.  All
    guards lie inside the allocation, so an access one row or one strip out of range cannot fault: a stray READ returns NaN
    (harmless when masked, a NaN / a bitwise mismatch in the result when used), a stray WRITE is found by check()."""

    def __init__(self, dev, specs, row_floats=0):
        import torch
        self.guard = -(-max(GUARD_MIN_BYTES, 2 * 4 * int(row_floats)) // 256) * 256
        self.where, cur = {}, 0                      # name -> (first word, words, shape or None, bytes)
        for name, shape, res in specs:
            assert name not in self.where, name
            cur = -(-(cur + self.guard) // 256) * 256
            if res == "ws":
                nbytes, shape = int(shape), None
                assert nbytes % 4 == 0
            else:
                assert res in (0, 4, 8, 12), res
                cur += 256 + res                     # (the 256: the guard in front never shrinks below self.guard)
                nbytes = 4 * int(np.prod(shape, dtype=np.int64))
            self.where[name] = (cur // 4, nbytes // 4, tuple(shape) if shape is not None else None, nbytes)
            cur += nbytes
        total = -(-(cur + self.guard) // 256) * 256
        self._block = torch.full((total // 4 + 64,), SENTINEL, dtype=torch.int32, device=dev)      # (+ 256 bytes: any allocator will do)
        skip = (-self._block.data_ptr() % 256) // 4
        self.words = self._block[skip:skip + total // 4]
        assert self.words.data_ptr() % 256 == 0
        self.is_guard = torch.ones((total // 4,), dtype=torch.bool, device=dev)
        for first, n, _, _ in self.where.values():
            self.is_guard[first:first + n] = False
        self._snap = {}
        for name, (_, _, shape, _) in self.where.items():      # the placement is what was asked for
            assert shape is not None or self.ptr(name) % 256 == 0, name

    def ptr(self, name):
        return self.words.data_ptr() + 4 * self.where[name][0]

    def nbytes(self, name):
        return self.where[name][3]

    def raw(self, name):
        """the buffer as int32 words (a view)"""
        first, n, _, _ = self.where[name]
        return self.words[first:first + n]

    def view(self, name):
        """the buffer as a float32 array of its shape (a contiguous view: what the bindings accept)"""
        import torch
        first, n, shape, _ = self.where[name]
        t = self.words[first:first + n].view(torch.float32)
        return t if shape is None else t.view(shape)

    def set(self, name, a):
        import torch
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        self.view(name).copy_(a.to(self.words.device).reshape(self.view(name).shape))
        return self.view(name)

    def fill_bits(self, name, word=SENTINEL):
        """every 32-bit word of the buffer = `word` (an int in [0, 2^32))"""
        self.raw(name).fill_(word - (1 << 32) if word >= (1 << 31) else word)

    def fill(self, name, value):
        self.view(name).fill_(value)

    def bits(self, name):
        """host copy of the buffer's words, shaped like the array"""
        first, n, shape, _ = self.where[name]
        a = self.raw(name).cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)

    def snapshot(self, name):
        self._snap[name] = self.raw(name).clone()

    def unchanged(self, name):
        import torch
        assert torch.equal(self._snap[name], self.raw(name)), "input %r was written to by the call" % name

    def sentinels_left(self, name):
        """how many words of the buffer still hold the sentinel (an "overwritten" output has none)"""
        return int((self.raw(name) == SENTINEL).sum().item())

    def check(self, what=""):
        """every guard word still holds the sentinel; otherwise names the nearest buffer, the side and the first offending byte"""
        bad = (self.words != SENTINEL) & self.is_guard
        if not bool(bad.any().item()):
            return
        idx = bad.nonzero().flatten().cpu().numpy()
        names = list(self.where)
        first = np.array([self.where[n][0] for n in names])
        end = first + np.array([self.where[n][1] for n in names])
        # every damaged word belongs to the nearest buffer edge: the end of the buffer in front of it or the start of the one behind
        k_after = np.searchsorted(first, idx, side="right") - 1          # the buffer that starts before the word (-1: none)
        msgs = []
        for k, name in enumerate(names):
            d_after = idx[k_after == k] - end[k]                         # words past the end of buffer k ...
            nxt = first[k + 1] if k + 1 < len(names) else None
            if nxt is not None:
                d_after = d_after[d_after < (nxt - idx[k_after == k])]   # ... unless the next buffer's start is nearer
            d_before = first[k] - idx[k_after == k - 1] if k > 0 else first[k] - idx[k_after == -1]
            if k > 0:
                d_before = d_before[d_before <= idx[k_after == k - 1] - end[k - 1]]
            if d_after.size:
                msgs.append("%s: %d words written AFTER it, first at byte offset +%d past its end (byte %d of the buffer)"
                            % (name, d_after.size, 4 * int(d_after.min()), 4 * int(d_after.min() + end[k] - first[k])))
            if d_before.size:
                msgs.append("%s: %d words written BEFORE it, nearest at byte offset -%d" % (name, d_before.size, 4 * int(d_before.min())))
        raise AssertionError("%s guard words overwritten (%d in all): %s" % (what, idx.size, "; ".join(msgs)))
