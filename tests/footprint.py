"""Footprint frames: hold a device call to the words it may write (test infrastructure, not a conftest).

The parity tests size an output exactly and download only it, so a write past its end, in front of it or into an operand of an
out-of-place call lands where nobody looks.  A Frame puts every named part of one call -- operands, plaintexts, output -- into ONE
device allocation,

    zone | part | zone | part | ... | zone

with every part starting on a 16-byte boundary and every zone at least `zone_words` long, so a stray write of up to a zone's
length lands in memory the test owns and cannot fault.  Zones, and parts given as a word count (outputs), are pre-filled with
SENTINEL ^ word_index: the top bits are set, so it is no residue of any prime below 2^60 (and a NaN-free but absurd double), and it
differs from word to word, so a displaced copy of a valid word or of another sentinel is seen too.

    frame = Frame(g, [("a", a), ("b", b), ("out", a.size)], zone_words)
    g.op("add", frame.ptr("a"), frame.ptr("b"), frame.ptr("out"), ...)
    res = frame.check(written={"out"})     # ONE download of the whole frame
    res.changed      {name: (words changed, first offset)} over every zone and every part not in `written`; empty = clean
    res.unwritten    {name: (sentinel words left, first offset)} over the parts in `written` that were pre-filled
    res.part("out")  the words of a written part, for the comparison with the oracle

`g` is anything with upload(array) -> buffer (.ptr a ctypes.c_void_p, .free()) and download(buffer, shape) -> uint64 array:
abc_amd.capi.Context, or HostDevice below, numpy standing in for the device (tests/test_footprint_frame.py).
"""
import ctypes as C

import numpy as np

SENTINEL = 0xFACEFEEDC0DE0000  # >= 2^63: above every coefficient prime, and the index below 2^32 never reaches the set bits


def sentinel_words(first_index, words):
    """SENTINEL ^ index for `words` consecutive word indices"""
    return np.uint64(SENTINEL) ^ np.arange(first_index, first_index + words, dtype=np.uint64)


def zone_words_for(n, *operand_shapes):
    """the larger of one ciphertext of the call's widest operand ([count][size][nl][N] -> size * nl * N) and 2 * N"""
    widest = max([int(np.prod(s[1:])) if len(s) > 1 else int(np.prod(s)) for s in operand_shapes] + [0])
    return max(widest, 2 * int(n))


def _as_words(value):
    a = np.ascontiguousarray(value)
    if a.dtype.itemsize != 8:
        raise ValueError("a frame part holds 8-byte words")
    return a.reshape(-1).view(np.uint64)


class Result:
    def __init__(self, frame, image, written):
        self._frame, self._image = frame, image
        self.changed, self.unwritten = {}, {}
        for name, (off, words) in frame.zones.items():
            self._compare(self.changed, name, image[off:off + words], frame.initial[off:off + words], np.not_equal)
        for name, (off, words) in frame.parts.items():
            got, was = image[off:off + words], frame.initial[off:off + words]
            if name not in written:
                self._compare(self.changed, name, got, was, np.not_equal)
            elif name in frame.prefilled:
                self._compare(self.unwritten, name, got, was, np.equal)

    @staticmethod
    def _compare(into, name, got, was, rel):
        hit = np.flatnonzero(rel(got, was))
        if len(hit):
            into[name] = (int(len(hit)), int(hit[0]))

    def part(self, name, shape=None, dtype=np.uint64):
        off, words = self._frame.parts[name]
        out = self._image[off:off + words].view(dtype)
        return out if shape is None else out.reshape(shape)

    @property
    def clean(self):
        return not self.changed and not self.unwritten


class Frame:
    def __init__(self, g, parts, zone_words):
        """parts: [(name, array of 8-byte words -- uploaded as it is -- or a word count -- pre-filled with the sentinel)], in order"""
        zone_words = (int(zone_words) + 1) & ~1
        if zone_words < 2:
            raise ValueError("a zone is at least one 16-byte unit")
        self.g, self.parts, self.zones, self.prefilled, self.order = g, {}, {}, set(), []
        contents, at = {}, 0
        for k, (name, value) in enumerate(parts):
            if name in self.parts:
                raise ValueError("part named twice: " + name)
            # the zone in front of a part runs from the end of the part before it (odd lengths: one word more) to the part's start
            start = (at + zone_words + 1) & ~1
            self.zones["zone%d" % k] = (at, start - at)
            words = int(value) if np.ndim(value) == 0 and not isinstance(value, np.ndarray) else None
            if words is None:
                contents[name] = _as_words(value)
                words = contents[name].size
            else:
                self.prefilled.add(name)
            self.parts[name] = (start, words)
            self.order.append(name)
            at = start + words
        end = (at + zone_words + 1) & ~1
        self.zones["zone%d" % len(parts)] = (at, end - at)
        self.words = end
        self.initial = sentinel_words(0, end)
        for name, data in contents.items():
            off, words = self.parts[name]
            self.initial[off:off + words] = data
        self.initial.setflags(write=False)
        self.buf = g.upload(self.initial)
        self.base = self.buf.ptr.value

    def offset(self, name):
        """word offset of a part in the frame"""
        return self.parts[name][0]

    def ptr(self, name, word=0):
        """the interior device pointer of a part (16-byte aligned at word 0)"""
        return C.c_void_p(self.base + 8 * (self.parts[name][0] + int(word)))

    def zone_before(self, name):
        return "zone%d" % self.order.index(name)

    def zone_after(self, name):
        return "zone%d" % (self.order.index(name) + 1)

    def check(self, written=()):
        image = self.g.download(self.buf, (self.words,))
        return Result(self, image, set(written))

    def close(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


class HostDevice:
    """numpy standing in for the device: upload copies into host memory whose address is the 'device pointer'"""

    class _Buffer:
        def __init__(self, mem):
            self.mem, self.nbytes = mem, mem.nbytes
            self.ptr = C.c_void_p(mem.ctypes.data)

        def free(self):
            self.mem = None

    def upload(self, arr):
        return self._Buffer(np.array(_as_words(arr), dtype=np.uint64))

    def download(self, buf, shape):
        return buf.mem.reshape(shape).copy()

    @staticmethod
    def words_at(ptr, words):
        """what a 'kernel' of the self-tests writes through: the `words` words at a pointer Frame.ptr returned"""
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(words,))
