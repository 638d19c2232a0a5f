"""How results reach a caller: operands and results in torch tensors, the context on a torch.cuda.Stream (abc_hip_set_stream), and
no host synchronisation between the caller's producer, the C-ABI call and the caller's consumer.

The header's contract (include/abc_hip.h, conventions block and abc_hip_set_stream): a d_ pointer may be any HIP allocation; work is
enqueued on the context's stream; a caller that passes a real stream handle gets ordering against its own work on that stream; the
internal lanes fork from and join it inside each call.  Part 1 is parity on foreign memory and a foreign stream, synchronised
normally.  Part 2 is the ordering: behind a device-side spin the inputs are copied device to device into operand tensors that hold
zeros, the call is issued, the result is cloned -- all on the torch stream, the host waits only afterwards, with torch's own
synchronize.  A call not ordered behind the stream reads zeros; lanes not joined into it let the clone run before the result exists;
either way the snapshot differs from the oracle.  Part 3 is the control that says whether such an error could show in this process
at all, part 4 switches streams and contexts.  Every assertion is bit-equality with the CPU oracle (hoisted rotations: with the
definition composed from oracle calls, tests/hoisted_spec.py)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hoisted_spec import hoisted_reference  # noqa: E402

pytestmark = pytest.mark.gpu

N12, N14 = 1 << 12, 1 << 14
CHAIN = [50, 40, 50]  # two data limbs and the special prime
STEPS = [1, -1, 8]    # Galois keys: 1 and 8 rotate directly, 7 = 8 - 1 takes the NAF chain (two key switches in one call)
LEAN = "split14 front=lean pack=1 main=split4"
B12, B14 = 3, 9       # B14 with ABC_HIP_CHUNK=2: chunks of 2, 2, 2, 2, 1 alternating over two lanes


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s: got %d want %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _dev(arr):
    """uint64 residues (every prime is below 2^63) or int64 values -> a torch.int64 CUDA tensor, bit for bit"""
    arr = np.array(arr, order="C")  # a copy: the shared references are read-only, which torch.from_numpy does not take
    return torch.from_numpy(arr.view(np.int64) if arr.dtype == np.uint64 else arr).to("cuda")


def _host(t, dtype=np.uint64):
    return t.cpu().numpy().view(dtype)


def _ptr(t):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int64
    return C.c_void_p(t.data_ptr())


def _sz(count):
    return C.c_size_t(count)


@contextlib.contextmanager
def _environ(settings):
    old = {k: os.environ.get(k) for k in settings}
    os.environ.update(settings)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _load(capi, o):
    g = capi.Context(capi.CKKS if o.scheme == 2 else capi.BFV, o.n, o.primes, o.t)
    g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
    return g


def _random_cts(primes, nl, n, count, rng):
    return np.stack([np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in primes[:nl]], axis=1) for _ in range(count)])


class Rig:
    """An oracle with Galois keys for STEPS, a device context with the same keys on a torch stream of its own, a batch of inputs
    and the references computed so far: computed once, shared by the tests of the module, never changed."""

    def __init__(self, om, capi, scheme, n, primes, t, count, seed, env=None):
        self.capi = capi
        self.o = om.Oracle(scheme, n, primes, t)
        self.elts = [self.o.elt_from_step(s) for s in STEPS]
        self.o.keygen(seed, elts=self.elts)
        self.env = dict(env or {})
        self.g = self.new_context()
        self.stream = torch.cuda.Stream()
        self.g.set_stream(self.stream.cuda_stream)
        self.n, self.L, self.B, self.primes = n, self.o.L, count, list(primes)
        rng = np.random.default_rng(n + count)
        if scheme == om.CKKS:
            self.a, self.b = _random_cts(primes, self.L, n, count, rng), _random_cts(primes, self.L, n, count, rng)
        else:  # real encryptions: the noise budget of a random ciphertext is zero whatever the kernel does
            enc = lambda s: self.o.encrypt(self.o.encode(rng.integers(0, t, n)), s)  # noqa: E731
            self.a, self.b = np.stack([enc(10 + i) for i in range(count)]), np.stack([enc(50 + i) for i in range(count)])
        for x in (self.a, self.b):
            x.setflags(write=False)
        self._want = {}

    def new_context(self):
        with _environ(self.env):  # the path switches are read when a context is created
            return _load(self.capi, self.o)

    def want(self, key, fn):
        if key not in self._want:
            self._want[key] = np.ascontiguousarray(fn())
            self._want[key].setflags(write=False)
        return self._want[key]

    def each(self, key, fn, *batches):
        """fn over the rows of the batches, stacked"""
        return self.want(key, lambda: np.stack([fn(*rows) for rows in zip(*batches)]))

    # the references more than one test needs
    def mul(self):
        return self.each("mul_relin", self.o.mul_relin, self.a, self.b)

    def rot(self, steps):
        return self.each(("rotate", steps), lambda x: self.o.rotate(x, steps), self.a)

    def chain(self):  # rotate(a * b, 1) + a
        return self.each("chain", lambda m, x: self.o.add(self.o.rotate(m, 1), x), self.mul(), self.a)

    def hoisted(self):  # [2][B][2][nl][N]
        return self.want("hoisted", lambda: np.stack([np.stack([hoisted_reference(self.o, x, e) for x in self.a]) for e in self.elts[::2]]))

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def ckks12(oracle_mod, capi):
    rig = Rig(oracle_mod, capi, oracle_mod.CKKS, N12, oracle_mod.create_primes(N12, CHAIN), 0, B12, 0x57E0)
    yield rig
    rig.close()


@pytest.fixture(scope="module")
def bfv12(oracle_mod, capi):
    primes = oracle_mod.default_bfv_primes(N12)
    rig = Rig(oracle_mod, capi, oracle_mod.BFV, N12, primes, oracle_mod.plain_modulus_batching(N12, 20), B12, 0x57E1)
    yield rig
    rig.close()


@pytest.fixture(scope="module")
def ckks14(oracle_mod, capi):
    """N = 2^14, nl = 2: the smallest shape at which the two internal lanes exist"""
    rig = Rig(oracle_mod, capi, oracle_mod.CKKS, N14, oracle_mod.create_primes(N14, CHAIN), 0, B14, 0x57E2,
              env={"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": "2"})
    yield rig
    rig.close()


def _routes14(g):
    assert g.route("mul_relin", 2, B14) == LEAN
    assert g.route("rotate", 2, B14) == "fold " + LEAN


def _sync_call(rig, fn):
    """part 1: inputs and outputs in torch tensors, the call on the torch stream, synchronised normally"""
    with torch.cuda.stream(rig.stream):
        res = fn()
    rig.stream.synchronize()
    return res


def _zeros(*shape):
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity on foreign memory and a foreign stream
# ---------------------------------------------------------------------------------------------------------------------
def _check_evaluator_ops(rig, scheme_name):
    g, o, B, L, n = rig.g, rig.o, rig.B, rig.L, rig.n
    a, b = _dev(rig.a), _dev(rig.b)
    torch.cuda.synchronize()
    cnt = _sz(B)

    def run(name, out, *args):
        _sync_call(rig, lambda: g.op(name, *args))
        return _host(out)

    out = torch.empty_like(a)
    _same(scheme_name + " add", run("add", out, _ptr(a), _ptr(b), _ptr(out), 2, L, cnt), rig.each("add", o.add, rig.a, rig.b))
    _same(scheme_name + " sub", run("sub", out, _ptr(a), _ptr(b), _ptr(out), 2, L, cnt), rig.each("sub", o.sub, rig.a, rig.b))
    _same(scheme_name + " negate", run("negate", out, _ptr(a), _ptr(out), 2, L, cnt), rig.each("negate", o.negate, rig.a))
    out3 = _zeros(B, 3, L, n)
    want3 = rig.each("multiply", o.multiply, rig.a, rig.b)
    _same(scheme_name + " multiply", run("multiply", out3, _ptr(a), _ptr(b), _ptr(out3), L, cnt), want3)
    in3 = _dev(want3)
    _same(scheme_name + " relinearize", run("relinearize", out, _ptr(in3), _ptr(out), L, cnt), rig.mul())
    out.zero_()
    _same(scheme_name + " mul_relin", run("mul_relin", out, _ptr(a), _ptr(b), _ptr(out), L, cnt), rig.mul())
    _same(scheme_name + " rotate 1 (direct)", run("rotate", out, _ptr(a), _ptr(out), L, 1, cnt), rig.rot(1))
    _same(scheme_name + " rotate 7 (NAF)", run("rotate", out, _ptr(a), _ptr(out), L, 7, cnt), rig.rot(7))
    elts = (C.c_uint32 * 2)(*rig.elts[::2])
    outh = _zeros(2, B, 2, L, n)
    _same(scheme_name + " apply_galois_hoisted", run("apply_galois_hoisted", outh, _ptr(a), _ptr(outh), L, elts, 2, B), rig.hoisted())
    cp = _zeros(*a.shape)
    _same(scheme_name + " memcpy_d2d", run("memcpy_d2d", cp, _ptr(cp), _ptr(b), _sz(rig.b.nbytes)), rig.b)


def _check_plain_ops(rig, scheme_name, plains):
    """plains uint64 [B][per]: row 0 is the broadcast plaintext of the stride-0 calls"""
    g, o, B, L = rig.g, rig.o, rig.B, rig.L
    a, pl = _dev(rig.a), _dev(plains)
    torch.cuda.synchronize()
    out = torch.empty_like(a)
    per = plains[0].size
    for name, ofn in (("multiply_plain", o.multiply_plain), ("add_plain", o.add_plain)):
        for stride in (0, per):
            _sync_call(rig, lambda: g.op(name, _ptr(a), _ptr(pl), _sz(stride), _ptr(out), 2, L, _sz(B)))
            want = rig.each((name, stride), lambda x, p: ofn(x, p), rig.a, plains if stride else [plains[0]] * B)
            _same("%s %s stride %d" % (scheme_name, name, stride), _host(out), want)


def _ckks_plains(rig):
    """uint64 [B][L][N], NTT-form residues: one plaintext per ciphertext"""
    rng = np.random.default_rng(12)
    return rig.want("plains", lambda: np.stack([np.stack([rng.integers(0, q, rig.n, dtype=np.uint64) for q in rig.primes[:rig.L]])
                                                for _ in range(rig.B)]))


def _check_ntt_limbs(rig, scheme_name):
    g, o, L, n = rig.g, rig.o, rig.L, rig.n
    rng = np.random.default_rng(3)
    polys = np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in rig.primes[:L]]) for _ in range(3)])
    fwd = np.stack([np.stack([o.ntt(j, p[j]) for j in range(L)]) for p in polys])
    d = _dev(polys)
    torch.cuda.synchronize()
    _sync_call(rig, lambda: g.op("ntt_limbs", _ptr(d), L, _sz(3), 0))
    _same(scheme_name + " ntt_limbs forward", _host(d), fwd)
    _sync_call(rig, lambda: g.op("ntt_limbs", _ptr(d), L, _sz(3), 1))
    _same(scheme_name + " ntt_limbs inverse", _host(d), polys)


def test_parity_ckks12_on_torch_tensors_and_stream(ckks12):
    rig = ckks12
    g, o, B, L, n = rig.g, rig.o, rig.B, rig.L, rig.n
    _check_evaluator_ops(rig, "ckks12")
    _check_plain_ops(rig, "ckks12", _ckks_plains(rig))
    _check_ntt_limbs(rig, "ckks12")
    a = _dev(rig.a)
    torch.cuda.synchronize()
    low = _zeros(B, 2, L - 1, n)
    _sync_call(rig, lambda: g.op("rescale", _ptr(a), _ptr(low), 2, L, _sz(B)))
    _same("ckks12 rescale", _host(low), rig.each("rescale", o.rescale, rig.a))
    _sync_call(rig, lambda: g.op("mod_switch", _ptr(a), _ptr(low), 2, L, _sz(B)))
    _same("ckks12 mod_switch", _host(low), rig.each("mod_switch", o.mod_switch, rig.a))
    pt = _zeros(B, L, n)
    _sync_call(rig, lambda: g.op("decrypt", _ptr(a), 2, L, _ptr(pt), _sz(B)))
    _same("ckks12 decrypt", _host(pt), rig.each("decrypt", o.decrypt, rig.a))


def test_parity_bfv12_on_torch_tensors_and_stream(bfv12):
    rig = bfv12
    g, o, B, L, n = rig.g, rig.o, rig.B, rig.L, rig.n
    _check_evaluator_ops(rig, "bfv12")
    rng = np.random.default_rng(13)
    values = rng.integers(-(rig.o.t // 2), rig.o.t // 2, size=(B, n), dtype=np.int64)
    plains = np.stack([o.encode(v) for v in values])
    _check_plain_ops(rig, "bfv12", plains)
    _check_ntt_limbs(rig, "bfv12")
    a, vals = _dev(rig.a), _dev(values)
    torch.cuda.synchronize()
    pt = _zeros(B, n)
    _sync_call(rig, lambda: g.op("decrypt", _ptr(a), 2, L, _ptr(pt), _sz(B)))
    _same("bfv12 decrypt", _host(pt), rig.each("decrypt", o.decrypt, rig.a))
    enc = _zeros(B, n)
    _sync_call(rig, lambda: g.op("batch_encode", _ptr(vals), _ptr(enc), _sz(B)))
    _same("bfv12 batch_encode", _host(enc), plains)
    dec = _zeros(B, n)
    _sync_call(rig, lambda: g.op("batch_decode", _ptr(enc), _ptr(dec), _sz(B)))
    _same("bfv12 batch_decode", _host(dec, np.int64), np.stack([o.decode(p) for p in plains]))
    budget = np.full(B, -1, dtype=np.int32)
    _sync_call(rig, lambda: g.op("noise_budget", _ptr(a), 2, L, budget.ctypes.data_as(C.POINTER(C.c_int)), _sz(B)))
    want = np.array([o.noise_budget(x) for x in rig.a], dtype=np.int32)
    assert want.min() > 0  # fresh encryptions: the comparison is not of zeros
    _same("bfv12 noise_budget", budget, want)


def test_parity_ckks14_two_lanes_on_torch_tensors_and_stream(ckks14):
    rig = ckks14
    g, B, L = rig.g, rig.B, rig.L
    _routes14(g)
    a, b = _dev(rig.a), _dev(rig.b)
    out = torch.empty_like(a)
    torch.cuda.synchronize()
    _sync_call(rig, lambda: g.op("mul_relin", _ptr(a), _ptr(b), _ptr(out), L, _sz(B)))
    _same("ckks14 mul_relin", _host(out), rig.mul())
    _sync_call(rig, lambda: g.op("rotate", _ptr(a), _ptr(out), L, 1, _sz(B)))
    _same("ckks14 rotate", _host(out), rig.rot(1))
    _sync_call(rig, lambda: g.op("mul_relin", _ptr(a), _ptr(b), _ptr(a), L, _sz(B)))
    _same("ckks14 mul_relin, out aliasing a", _host(a), rig.mul())


def test_parity_on_a_view_at_a_storage_offset(ckks12):
    """big[1:] of a [B + 1, ...] tensor: contiguous, but its pointer is not the start of an allocation -- as input and as output"""
    rig = ckks12
    g, B, L, n = rig.g, rig.B, rig.L, rig.n
    big_in, big_out = _zeros(B + 1, 2, L, n), _zeros(B + 1, 2, L, n)
    a, out, b = big_in[1:], big_out[1:], _dev(rig.b)
    a.copy_(_dev(rig.a))
    assert a.storage_offset() == 2 * L * n and out.storage_offset() == 2 * L * n and a.data_ptr() == big_in.data_ptr() + 16 * L * n
    torch.cuda.synchronize()
    _sync_call(rig, lambda: g.op("mul_relin", _ptr(a), _ptr(b), _ptr(out), L, _sz(B)))
    _same("mul_relin on views", _host(out), rig.mul())
    assert not _host(big_out[0]).any()  # the row in front of the view is untouched
    _sync_call(rig, lambda: g.op("rotate", _ptr(a), _ptr(out), L, 7, _sz(B)))
    _same("rotate (NAF) on views", _host(out), rig.rot(7))
    assert not _host(big_out[0]).any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ordering with no host synchronisation between producer, call and consumer
# ---------------------------------------------------------------------------------------------------------------------
_SPIN = {}
MIN_SPIN_MS = 25.0  # floor of the spin: also covers the host time it takes to issue the copies and the call's launches


def _cycles_per_ms():
    """torch.cuda._sleep counts in a unit nobody has measured here: time a fixed spin with torch events, once per process"""
    if "rate" not in _SPIN:
        probe = 5_000_000
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(probe)  # the first launch loads the kernel
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
        s.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, "torch.cuda._sleep(%d) took %.4f ms: too short to calibrate" % (probe, ms)
        _SPIN["rate"] = probe / ms
        print("spin calibration: torch.cuda._sleep(%d) took %.3f ms" % (probe, ms))
    return _SPIN["rate"]


def _spin_cycles(what, op_ms):
    spin_ms = max(10.0 * op_ms, MIN_SPIN_MS)  # at least ten times the op: a mis-ordered call only has to read its inputs before the spin ends
    print("%s: op %.3f ms eagerly, spin %.1f ms" % (what, op_ms, spin_ms))
    return int(spin_ms * _cycles_per_ms())


def _timed(g, fn):
    g.timer_start()
    fn()
    return g.timer_stop()


def _ordered(what, stream, timer_ctx, srcs, shapes, call, tensors=None, after=None):
    """The producer / call / consumer sequence of part 2.  srcs: device tensors holding the real inputs; shapes: of the further
    tensors (results, temporaries).  call(*operands, *further) issues the C-ABI calls and returns the tensor holding the result.
    Everything is issued on `stream` with no host wait in between; the host waits with torch's synchronize, after the snapshot.
    tensors: operands and further tensors made by the caller (a recorded circuit has their addresses baked in); after: a further
    wait once the snapshot is taken and `stream` is drained (the control of part 3, whose context is not on `stream`)."""
    ops = list(tensors[:len(srcs)]) if tensors else [torch.zeros_like(s) for s in srcs]
    rest = list(tensors[len(srcs):]) if tensors else [_zeros(*shape) for shape in shapes]
    torch.cuda.synchronize()
    # once eagerly: scratch growth and first-use key mirrors synchronise the host and would hide an ordering error; then the timing
    with torch.cuda.stream(stream):
        call(*ops, *rest)
    torch.cuda.synchronize()
    op_ms = _timed(timer_ctx, lambda: call(*ops, *rest))
    torch.cuda.synchronize()
    for t in ops + rest:
        t.zero_()
    torch.cuda.synchronize()
    cycles = _spin_cycles(what, op_ms)
    spun = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        spun.record()
        for t, s in zip(ops, srcs):
            t.copy_(s, non_blocking=True)
        res = call(*ops, *rest)
        issued_in_time = not spun.query()  # no wait: did the host get this far while the device was still spinning?
        snap = res.clone()
    stream.synchronize()
    if after is not None:
        after()
    assert issued_in_time, "%s: the spin had ended before the call was issued: the run proves nothing" % what
    return _host(snap)


def _srcs(rig):
    t = _dev(rig.a), _dev(rig.b)
    torch.cuda.synchronize()
    return t


def _run_ordered(rig, what, srcs, shapes, call, stream=None, tensors=None):
    return _ordered(what, stream or rig.stream, rig.g, srcs, shapes, call, tensors=tensors)


def _ct_shape(rig, nl=None):
    return (rig.B, 2, rig.L if nl is None else nl, rig.n)


def test_ordered_ckks14_two_lanes_mul_relin(ckks14):
    rig = ckks14
    g, L, cnt = rig.g, rig.L, _sz(rig.B)
    _routes14(g)

    def call(a, b, out):
        g.op("mul_relin", _ptr(a), _ptr(b), _ptr(out), L, cnt)
        return out
    _same("ordered two-lane mul_relin", _run_ordered(rig, "ckks14 mul_relin", _srcs(rig), [_ct_shape(rig)], call), rig.mul())

    def in_place(a, b):
        g.op("mul_relin", _ptr(a), _ptr(b), _ptr(a), L, cnt)
        return a
    _same("ordered two-lane mul_relin, out aliasing a", _run_ordered(rig, "ckks14 mul_relin in place", _srcs(rig), [], in_place), rig.mul())


def test_ordered_ckks14_two_lanes_rotate(ckks14):
    rig = ckks14
    g, L, cnt = rig.g, rig.L, _sz(rig.B)
    _routes14(g)

    def call(a, out):
        g.op("rotate", _ptr(a), _ptr(out), L, 1, cnt)
        return out
    _same("ordered two-lane rotate", _run_ordered(rig, "ckks14 rotate", _srcs(rig)[:1], [_ct_shape(rig)], call), rig.rot(1))


def test_ordered_ckks12_single_ops(ckks12):
    rig = ckks12
    g, o, B, L, n, cnt = rig.g, rig.o, rig.B, rig.L, rig.n, _sz(rig.B)
    a_src, b_src = _srcs(rig)

    def add(a, b, out):
        g.op("add", _ptr(a), _ptr(b), _ptr(out), 2, L, cnt)
        return out
    _same("ordered add", _run_ordered(rig, "ckks12 add", [a_src, b_src], [_ct_shape(rig)], add), rig.each("add", o.add, rig.a, rig.b))

    plains = _ckks_plains(rig)  # those of the parity test: the reference is shared
    per = plains[0].size
    p_src = _dev(plains)

    def multiply_plain(a, p, out):
        g.op("multiply_plain", _ptr(a), _ptr(p), _sz(per), _ptr(out), 2, L, cnt)
        return out
    _same("ordered multiply_plain", _run_ordered(rig, "ckks12 multiply_plain", [a_src, p_src], [_ct_shape(rig)], multiply_plain),
          rig.each(("multiply_plain", per), o.multiply_plain, rig.a, plains))

    def rescale(a, out):
        g.op("rescale", _ptr(a), _ptr(out), 2, L, cnt)
        return out
    _same("ordered rescale", _run_ordered(rig, "ckks12 rescale", [a_src], [_ct_shape(rig, L - 1)], rescale), rig.each("rescale", o.rescale, rig.a))

    def decrypt(a, out):
        g.op("decrypt", _ptr(a), 2, L, _ptr(out), cnt)
        return out
    _same("ordered decrypt", _run_ordered(rig, "ckks12 decrypt", [a_src], [(B, L, n)], decrypt), rig.each("decrypt", o.decrypt, rig.a))


def test_ordered_ckks12_key_switches(ckks12):
    rig = ckks12
    g, B, L, cnt = rig.g, rig.B, rig.L, _sz(rig.B)
    a_src = _srcs(rig)[0]
    elts = (C.c_uint32 * 2)(*rig.elts[::2])

    def hoisted(a, out):
        g.op("apply_galois_hoisted", _ptr(a), _ptr(out), L, elts, 2, B)
        return out
    _same("ordered apply_galois_hoisted", _run_ordered(rig, "ckks12 apply_galois_hoisted", [a_src], [(2,) + _ct_shape(rig)], hoisted), rig.hoisted())

    def naf(a, out):  # two key switches through the context's arenas in one call
        g.op("rotate", _ptr(a), _ptr(out), L, 7, cnt)
        return out
    _same("ordered rotate (NAF)", _run_ordered(rig, "ckks12 rotate NAF", [a_src], [_ct_shape(rig)], naf), rig.rot(7))


def _chain(g, L, cnt):
    """rotate(a * b, 1) + a through two caller-held temporaries, no synchronisation between the three calls"""
    def call(a, b, t1, t2, out):
        g.op("mul_relin", _ptr(a), _ptr(b), _ptr(t1), L, cnt)
        g.op("rotate", _ptr(t1), _ptr(t2), L, 1, cnt)
        g.op("add", _ptr(t2), _ptr(a), _ptr(out), 2, L, cnt)
        return out
    return call


@pytest.mark.parametrize("ring", ["ckks12", "ckks14"])
def test_ordered_three_op_chain(ring, request):
    rig = request.getfixturevalue(ring)
    call = _chain(rig.g, rig.L, _sz(rig.B))
    _same("ordered chain", _run_ordered(rig, ring + " chain", _srcs(rig), [_ct_shape(rig)] * 3, call), rig.chain())


def _replayed(rig, what, record_on_private_stream):
    """the chain recorded into a graph over fixed torch tensors, then replayed inside the producer / consumer sequence"""
    g, L, cnt = rig.g, rig.L, _sz(rig.B)
    chain = _chain(g, L, cnt)
    tensors = [_zeros(*_ct_shape(rig)) for _ in range(5)]  # a, b, t1, t2, out: the addresses the graph bakes in
    torch.cuda.synchronize()
    graph = None
    try:
        if record_on_private_stream:
            g.set_stream(None)
        chain(*tensors)  # once eagerly, on the stream the capture runs on
        g.sync()
        g.graph_begin()
        try:
            chain(*tensors)
        finally:
            graph = g.graph_end()
        g.set_stream(rig.stream.cuda_stream)

        def call(a, b, t1, t2, out):
            g.graph_launch(graph)
            return out
        got = _run_ordered(rig, what, _srcs(rig), [], call, tensors=tensors)
    finally:
        g.set_stream(rig.stream.cuda_stream)
        if graph is not None:
            g.graph_destroy(graph)
    return got


@pytest.mark.parametrize("ring", ["ckks12", "ckks14"])
def test_ordered_graph_recorded_on_the_torch_stream(ring, request):
    rig = request.getfixturevalue(ring)
    _same("ordered replay", _replayed(rig, ring + " graph (torch stream)", False), rig.chain())


@pytest.mark.parametrize("ring", ["ckks12", "ckks14"])
def test_ordered_graph_recorded_on_the_private_stream(ring, request):
    rig = request.getfixturevalue(ring)
    _same("ordered replay of a private-stream recording", _replayed(rig, ring + " graph (private stream)", True), rig.chain())


# ---------------------------------------------------------------------------------------------------------------------
# 3. is the ordering test sensitive in this process?
# ---------------------------------------------------------------------------------------------------------------------
def test_control_private_stream_reads_stale_inputs(ckks14):
    """The context is left on its private stream, which is ordered against nothing (header): behind the spin on the torch stream
    the call must run at once, on the zeros.  The two-lane call of part 2, once: a read of valid memory at the wrong time, not a
    fault.  A process has few hardware queues and a context alone owns five streams; two streams on one hardware queue serialise
    whatever the code says, and a missing dependency between them cannot show.  The call's kernels all run on the two lanes (chunks
    0, 2, 4 and chunks 1, 3), so the outcome is read per ciphertext: each one is the result for zeros (the stale read was observed)
    or the result for the real inputs (its lane was serialised behind the torch stream by the hardware); anything else fails.
    With no stale read at all the ordering tests were not sensitive in this process and the test skips, saying so."""
    rig = ckks14
    g, L, cnt = rig.g, rig.L, _sz(rig.B)
    _routes14(g)

    def call(a, b, out):
        g.op("mul_relin", _ptr(a), _ptr(b), _ptr(out), L, cnt)
        return out
    g.set_stream(None)
    try:  # both streams are synchronised: the torch stream by _ordered, the private one through the C ABI
        got = _ordered("control (private stream)", rig.stream, g, _srcs(rig), [_ct_shape(rig)], call, after=g.sync)
    finally:
        g.set_stream(rig.stream.cuda_stream)
    zero = np.zeros((2, L, rig.n), dtype=np.uint64)
    stale_row, real = rig.want("mul_relin of zeros", lambda: rig.o.mul_relin(zero, zero)), rig.mul()
    stale = [i for i in range(rig.B) if np.array_equal(got[i], stale_row)]
    serialised = [i for i in range(rig.B) if np.array_equal(got[i], real[i])]
    for i in range(rig.B):
        if i not in stale and i not in serialised:
            _same("control, ciphertext %d: neither the result for zeros nor the result for the real inputs" % i, got[i], stale_row)
    if not stale:
        pytest.skip("the private stream's lanes and the torch stream were serialised by the hardware: the ordering tests were not sensitive in this process")
    print("control: stale read observed on ciphertexts %s; serialised behind the torch stream by the hardware: %s" % (stale, serialised or "none"))


# ---------------------------------------------------------------------------------------------------------------------
# 4. switching streams
# ---------------------------------------------------------------------------------------------------------------------
def test_switching_between_two_torch_streams(ckks14):
    """the sequence on stream A, then on B after a cache-hit reallocation of the abc_hip_malloc temporary, on A again, and on the
    private stream (which is unordered: there the caller synchronises its producer before the call and the context after it)"""
    rig = ckks14
    g, L, cnt = rig.g, rig.L, _sz(rig.B)
    A, Bs = rig.stream, torch.cuda.Stream()
    nbytes = rig.a.nbytes
    want = rig.each("mul_rot", lambda m: rig.o.rotate(m, 1), rig.mul())
    tmp = [g.alloc(nbytes)]

    def call(a, b, out):  # mul_relin into the context-allocated temporary, rotate out of it
        g.op("mul_relin", _ptr(a), _ptr(b), tmp[0].ptr, L, cnt)
        g.op("rotate", tmp[0].ptr, _ptr(out), L, 1, cnt)
        return out
    try:
        _same("on A", _run_ordered(rig, "switch: A", _srcs(rig), [_ct_shape(rig)], call, stream=A), want)
        old, cached = tmp[0].ptr.value, g.cached_bytes()
        tmp[0].free()
        assert g.cached_bytes() == cached + nbytes
        g.set_stream(Bs.cuda_stream)
        tmp[0] = g.alloc(nbytes)
        assert tmp[0].ptr.value == old and g.cached_bytes() == cached  # a cache hit: the block crosses from A to B
        _same("on B", _run_ordered(rig, "switch: B", _srcs(rig), [_ct_shape(rig)], call, stream=Bs), want)
        g.set_stream(A.cuda_stream)
        _same("on A again", _run_ordered(rig, "switch: A again", _srcs(rig), [_ct_shape(rig)], call, stream=A), want)
        g.set_stream(None)
        a, b = _srcs(rig)
        out = _zeros(*_ct_shape(rig))
        with torch.cuda.stream(A):
            a2, b2 = a.clone(), b.clone()  # produced on A ...
        A.synchronize()                    # ... and synchronised by the caller, as the header demands for the private stream
        call(a2, b2, out)
        g.sync()
        with torch.cuda.stream(A):
            snap = out.clone()
        A.synchronize()
        _same("on the private stream", _host(snap), want)
    finally:
        g.set_stream(A.cuda_stream)
        tmp[0].free()


def test_two_contexts_on_one_torch_stream(ckks14):
    """ctx1.mul_relin writes the tensor ctx2.rotate reads, both contexts on the caller's stream, nothing between them"""
    rig = ckks14
    g1, L, cnt = rig.g, rig.L, _sz(rig.B)
    g2 = rig.new_context()
    try:
        g2.set_stream(rig.stream.cuda_stream)
        _routes14(g2)

        def call(a, b, mid, out):
            g1.op("mul_relin", _ptr(a), _ptr(b), _ptr(mid), L, cnt)
            g2.op("rotate", _ptr(mid), _ptr(out), L, 1, cnt)
            return out
        got = _run_ordered(rig, "two contexts", _srcs(rig), [_ct_shape(rig)] * 2, call)
        _same("ctx1.mul_relin -> ctx2.rotate", got, rig.each("mul_rot", lambda m: rig.o.rotate(m, 1), rig.mul()))
    finally:
        g2.close()


def test_set_stream_inside_a_capture_is_refused(ckks12, capi):
    """non-zero status, the capture stays usable: it still ends, and replays correctly on the stream it was recorded on"""
    rig = ckks12
    g, L, cnt = rig.g, rig.L, _sz(rig.B)
    other = torch.cuda.Stream()
    a, b = _srcs(rig)
    t1, t2, out = (_zeros(*_ct_shape(rig)) for _ in range(3))
    torch.cuda.synchronize()
    chain = _chain(g, L, cnt)
    chain(a, b, t1, t2, out)
    rig.stream.synchronize()
    g.graph_begin()
    try:
        g.op("mul_relin", _ptr(a), _ptr(b), _ptr(t1), L, cnt)
        with pytest.raises(capi.AbcHipError, match="not capturable"):
            g.set_stream(other.cuda_stream)
        with pytest.raises(capi.AbcHipError, match="not capturable"):
            g.set_stream(None)
        g.op("rotate", _ptr(t1), _ptr(t2), L, 1, cnt)
        g.op("add", _ptr(t2), _ptr(a), _ptr(out), 2, L, cnt)
    finally:
        graph = g.graph_end()
    try:
        for t in (t1, t2, out):
            t.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(rig.stream):
            g.graph_launch(graph)
            snap = out.clone()
        rig.stream.synchronize()
        _same("replay after the refused set_stream", _host(snap), rig.chain())
    finally:
        g.graph_destroy(graph)
