"""Recorded circuits (abc_hip_graph_*) against context changes made after recording.

A graph bakes raw device pointers into its kernel arguments: the scratch arenas, the key-switching keys and their mirrors
(fp64 twin, Shoup quotients).  The contract (include/abc_hip.h, graph comment): all of them outlive every graph that may
have recorded them, and a replay uses the keys current when it is launched.  Every check below compares the replay's
residues with the CPU oracle's, bit for bit, on inputs rewritten in place after recording.

Order matters for safety: every context first checks that the library reports its held-back buffers at all
(abc_hip_ctx_info 6), and wherever a change has to hold memory back, held_buffers() > 0 is asserted BEFORE the replay, so
that a library that frees the memory fails on the host instead of replaying over freed device memory.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 40
# name -> (scheme, n, chain bit sizes or None for BFVDefault(n), batch, environment)
CONFIGS = {
    "ckks14": ("ckks", 16384, [50, 40, 40, 40, 50], 12, {}),  # two lanes: split4 key switch, packed scratch, key twin
    "ckks14_no_split4": ("ckks", 16384, [50, 40, 40, 40, 50], 12, {"ABC_HIP_NO_SPLIT4": "1"}),
    "ckks14_no_key_twin": ("ckks", 16384, [50, 40, 40, 40, 50], 12, {"ABC_HIP_NO_KEY_TWIN": "1"}),
    "ckks14_60": ("ckks", 16384, [60, 40, 40, 40, 60], 12, {}),  # mixed chain: isplit for the 60-bit limbs
    "ckks15": ("ckks", 32768, [49, 49, 49, 49, 50], 4, {}),  # gsplit
    "bfv8192": ("bfv", 8192, None, 12, {}),  # bmul / bsplit at N = 2^13
    "bfv32768": ("bfv", 32768, None, 2, {}),  # integer key switch reading the key's Shoup mirror
}
KEY_SEED, NEW_KEY_SEED = 0x6A1, 0x6A2


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s" % (what, len(bad), got.size, tuple(bad[0])))


def _oracle(oracle_mod, scheme, n, bits, seed):
    if scheme == "ckks":
        o = oracle_mod.Oracle(oracle_mod.CKKS, n, oracle_mod.create_primes(n, bits))
    else:
        o = oracle_mod.Oracle.bfv_default(n)
    o.keygen(seed)
    return o


def _context(capi, o, seed, monkeypatch=None, env=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)  # read when the context is created
    g = capi.Context(capi.CKKS if o.scheme == 2 else capi.BFV, o.n, o.primes, o.t)
    # a library that does not count held-back buffers returns -1: stop here, before any replay
    assert g.held_buffers() >= 0
    assert g.held_buffers() == 0
    g.keygen(seed)  # device keygen(seed) == the oracle's keys (shared sampling spec)
    return g


class Rig:
    """r = add_plain(multiply_plain(rotate(a *** b, k) + a, p), p); CKKS: then rescale and mod_switch.  Batch B, own buffers."""

    def __init__(self, o, g, batch, k=3, seed=1):
        self.o, self.g, self.B, self.k = o, g, batch, k
        self.ckks = o.scheme == 2
        self.L, n = g.L, g.n
        rng = np.random.default_rng(seed)
        if self.ckks:
            self.plain = o.ckks_encode(rng.uniform(-1, 1, n // 2), SCALE)
        else:
            self.plain = o.encode(rng.integers(0, o.t, n))
        self.a, self.b = self._inputs(seed)
        self.da, self.db, self.dp = g.upload(self.a), g.upload(self.b), g.upload(self.plain)
        self.t = [g.alloc(self.a.nbytes) for _ in range(5)]
        self.out_shape = (batch, 2, self.L - 2 if self.ckks else self.L, n)
        self.out = g.alloc(int(np.prod(self.out_shape)) * 8)

    def _inputs(self, seed):
        o, n, rng = self.o, self.g.n, np.random.default_rng(seed + 1000)
        cts = []
        for i in range(2 * self.B):
            if self.ckks:
                pt = o.ckks_encode(rng.uniform(-1, 1, n // 2), SCALE)
            else:
                pt = o.encode(rng.integers(0, o.t, n))
            cts.append(o.encrypt(pt, seed * 7919 + i))
        return np.stack(cts[: self.B]), np.stack(cts[self.B:])

    def circuit(self):
        g, L, cb, t = self.g, self.L, C.c_size_t(self.B), self.t
        g.op("mul_relin", self.da.ptr, self.db.ptr, t[0].ptr, L, cb)
        g.op("rotate", t[0].ptr, t[1].ptr, L, self.k, cb)
        g.op("add", t[1].ptr, self.da.ptr, t[2].ptr, 2, L, cb)
        g.op("multiply_plain", t[2].ptr, self.dp.ptr, C.c_size_t(0), t[3].ptr, 2, L, cb)
        if self.ckks:
            g.op("add_plain", t[3].ptr, self.dp.ptr, C.c_size_t(0), t[4].ptr, 2, L, cb)
            g.op("rescale", t[4].ptr, t[0].ptr, 2, L, cb)  # t[0] is free again: [B][2][L-1][N]
            g.op("mod_switch", t[0].ptr, self.out.ptr, 2, L - 1, cb)
        else:
            g.op("add_plain", t[3].ptr, self.dp.ptr, C.c_size_t(0), self.out.ptr, 2, L, cb)

    def record(self):
        self.circuit()  # eager pass first: sizes the scratch, builds the key mirrors
        self.g.sync()
        self.g.graph_begin()
        self.circuit()
        return self.g.graph_end()

    def set_inputs(self, seed):
        """new contents in the same device buffers"""
        self.a, self.b = self._inputs(seed)
        for buf, arr in ((self.da, self.a), (self.db, self.b)):
            self.g.op("memcpy_h2d", buf.ptr, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes))

    def want(self, o=None):
        o = o or self.o
        res = []
        for a, b in zip(self.a, self.b):
            r = o.add(o.rotate(o.mul_relin(a, b), self.k), a)
            r = o.add_plain(o.multiply_plain(r, self.plain), self.plain)
            res.append(o.mod_switch(o.rescale(r)) if self.ckks else r)
        return np.stack(res)

    def replay(self, graph, o=None, what="replay", times=2):
        for _ in range(times):  # back to back, no sync in between
            self.g.graph_launch(graph)
        self.g.sync()
        _same(what, self.g.download(self.out, self.out_shape), self.want(o))

    def eager(self, o=None, what="eager"):
        self.circuit()
        self.g.sync()
        _same(what, self.g.download(self.out, self.out_shape), self.want(o))


def _random_cts(o, count, nl, seed):
    rng = np.random.default_rng(seed)
    cts = np.empty((count, 2, nl, o.n), dtype=np.uint64)
    for j in range(nl):
        cts[:, :, j, :] = rng.integers(0, o.primes[j], size=(count, 2, o.n), dtype=np.uint64)
    return cts


@pytest.fixture(scope="module")
def ckks14(oracle_mod):
    return _oracle(oracle_mod, "ckks", 16384, [50, 40, 40, 40, 50], KEY_SEED), \
        _oracle(oracle_mod, "ckks", 16384, [50, 40, 40, 40, 50], NEW_KEY_SEED)


# ---- a. replay parity across the kernel families the switches select ----
@pytest.mark.parametrize("name", list(CONFIGS))
def test_replay_with_new_inputs_matches_oracle(name, oracle_mod, capi, monkeypatch):
    scheme, n, bits, batch, env = CONFIGS[name]
    o = _oracle(oracle_mod, scheme, n, bits, KEY_SEED)
    g = _context(capi, o, KEY_SEED, monkeypatch, env)
    rig = Rig(o, g, batch)
    graph = rig.record()
    _same(name + " eager pass", g.download(rig.out, rig.out_shape), rig.want())
    rig.set_inputs(2)
    rig.replay(graph, what=name + " replay on new inputs")
    rig.set_inputs(3)
    rig.replay(graph, what=name + " second replay on new inputs")
    g.graph_destroy(graph)
    assert g.held_buffers() == 0
    g.close()


# ---- b. changes after recording ----
def test_scratch_growth_after_recording(ckks14, capi):
    """eager mul_relin and a NAF rotation on 4x the recorded batch grow the workspace and rotation arena 1 (arena)"""
    o, _ = ckks14
    g = _context(capi, o, KEY_SEED)
    rig = Rig(o, g, 4, k=3)  # step 3 = 4 - 1: two hops, the first through arena 1
    graph = rig.record()
    big = _random_cts(o, 16, g.L, 11)
    _same("eager mul_relin at 4x", g.mul_relin(big, big[::-1])[5], o.mul_relin(big[5], big[10]))
    _same("eager NAF rotate at 4x", g.rotate(big, 5)[7], o.rotate(big[7], 5))
    assert g.held_buffers() > 0  # the recorded workspace and arena were held back, not freed
    rig.set_inputs(4)
    rig.replay(graph, what="replay after scratch growth")
    g.graph_destroy(graph)
    assert g.held_buffers() == 0
    rig.eager(what="eager after the graph is gone")


def test_codec_and_encryption_after_recording(ckks14, capi):
    """ckks_decode / ckks_encode / decrypt / encrypt of large batches grow the workspace between replays (arena)"""
    o, _ = ckks14
    g = _context(capi, o, KEY_SEED)
    rig = Rig(o, g, 2)
    graph = rig.record()
    L, n = g.L, g.n
    rng = np.random.default_rng(5)
    plains = _random_cts(o, 64, L, 6)[:, 0]  # [64][L][N]: 32 MiB of decode scratch, the recording had 14
    dec = g.ckks_decode(plains, SCALE)
    for i in (0, 63):
        want = o.ckks_decode(plains[i], SCALE)
        assert np.abs(dec[i] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), i
    assert g.held_buffers() > 0
    rig.set_inputs(5)
    rig.replay(graph, what="replay after ckks_decode")
    vals = rng.uniform(-1, 1, (64, n // 2))
    enc = g.ckks_encode(vals, SCALE)
    assert np.abs(o.ckks_decode(enc[63], SCALE) - vals[63]).max() <= 1e-7  # the oracle decodes the device encoding
    rig.replay(graph, what="replay after ckks_encode")
    cts = _random_cts(o, 64, L, 7)
    _same("decrypt of a large batch", g.decrypt(cts)[40], o.decrypt(cts[40]))
    assert g.held_buffers() > 0
    rig.set_inputs(6)
    rig.replay(graph, what="replay after decrypt")
    enc_cts = g.encrypt(enc[:96 // 2].repeat(2, axis=0), seed=99)
    assert enc_cts.shape == (96, 2, L, n)
    # device encryption under a seed equals the oracle's (shared sampling spec) only per call: check it decrypts right instead
    assert np.allclose(o.ckks_decode(o.decrypt(enc_cts[95]), SCALE).real, vals[47], atol=1e-4)
    assert g.held_buffers() > 0
    rig.set_inputs(7)
    rig.replay(graph, what="replay after encrypt")
    g.graph_destroy(graph)
    assert g.held_buffers() == 0


def test_load_keys_after_recording(ckks14, capi):
    """load_keys(relin, galois) from another seed: the replay computes under the NEW keys (key, fp64 twin rewritten in place)"""
    o, o2 = ckks14
    g = _context(capi, o, KEY_SEED)
    rig = Rig(o, g, 12)
    graph = rig.record()
    g.load_keys(relin=o2.relin_key(), galois={e: o2.galois_key(e) for e in o2.galois_elts()})
    assert g.held_buffers() == 0  # rewritten in place: nothing to hold back
    rig.set_inputs(8)
    rig.replay(graph, o2, "replay under reloaded keys")
    rig.eager(o2, "eager under reloaded keys")
    g.load_keys(relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
    rig.replay(graph, o, "replay after loading the first keys back")
    g.graph_destroy(graph)


@pytest.mark.parametrize("name", ["ckks14", "bfv32768"])
def test_keygen_after_recording(name, oracle_mod, capi):
    """keygen(other seed) regenerates every key in its buffer and rebuilds the mirrors in place (key, twin, Shoup mirror)"""
    scheme, n, bits, batch, _ = CONFIGS[name]
    o = _oracle(oracle_mod, scheme, n, bits, KEY_SEED)
    g = _context(capi, o, KEY_SEED)
    rig = Rig(o, g, batch)
    graph = rig.record()
    o2 = _oracle(oracle_mod, scheme, n, bits, NEW_KEY_SEED)
    g.keygen(NEW_KEY_SEED)
    assert g.held_buffers() == 0  # the default Galois set is regenerated into the same buffers
    rig.set_inputs(9)
    rig.replay(graph, o2, name + " replay after keygen")
    rig.eager(o2, name + " eager after keygen")
    g.graph_destroy(graph)


def test_keygen_drops_a_loaded_galois_key_a_graph_uses(ckks14, capi):
    """a Galois key outside the default set, loaded by the caller and recorded, goes at keygen: held back (Galois buffer)"""
    o, _ = ckks14
    g = _context(capi, o, KEY_SEED)
    elt = 5  # not in the default set {2N-1, 3^(2^i), 3^-(2^i)}
    assert elt not in g.galois_elts()
    key = o.galois_key(o.galois_elts()[1])  # key-sized words: the oracle below switches with the same words
    g.load_keys(galois={elt: key})
    cts = _random_cts(o, 2, g.L, 12)
    want = []
    for ct in cts:  # apply_galois = (g(c0) + ks0, ks1), ks = KeySwitch(g(c1)) with the loaded key
        p0, p1 = o.galois_permute(ct[0], elt, True), o.galois_permute(ct[1], elt, True)
        want.append(o.add(np.stack([p0, np.zeros_like(p0)]), o.keyswitch(p1, key)))
    want = np.stack(want)
    d_in, d_out = g.upload(cts), g.alloc(cts.nbytes)
    cb = C.c_size_t(len(cts))
    g.op("apply_galois", d_in.ptr, d_out.ptr, g.L, C.c_uint32(elt), cb)
    g.sync()
    _same("eager apply_galois with the loaded key", g.download(d_out, cts.shape), want)
    g.graph_begin()
    g.op("apply_galois", d_in.ptr, d_out.ptr, g.L, C.c_uint32(elt), cb)
    graph = g.graph_end()
    g.keygen(NEW_KEY_SEED)
    assert elt not in g.galois_elts()
    assert g.held_buffers() > 0  # the dropped key and its mirror stay while the graph may read them
    g.op("negate", d_out.ptr, d_out.ptr, 2, g.L, cb)
    g.graph_launch(graph)
    g.sync()
    _same("replay over the dropped Galois key", g.download(d_out, cts.shape), want)
    g.graph_destroy(graph)
    assert g.held_buffers() == 0


def test_reload_env_after_recording(ckks14, capi, monkeypatch):
    """ABC_HIP_NO_KEY_TWIN=1 after recording: the graph still reads the twin, which a key reload must still refresh (twin)"""
    o, o2 = ckks14
    g = _context(capi, o, KEY_SEED)
    rig = Rig(o, g, 12)
    graph = rig.record()
    monkeypatch.setenv("ABC_HIP_NO_KEY_TWIN", "1")
    g.reload_env()
    rig.set_inputs(10)
    rig.replay(graph, what="replay after reload_env")
    rig.eager(what="eager without the twin")
    g.load_keys(relin=o2.relin_key(), galois={e: o2.galois_key(e) for e in o2.galois_elts()})
    rig.replay(graph, o2, "replay under reloaded keys, twins switched off for eager calls")
    rig.eager(o2, "eager under reloaded keys without the twin")
    g.graph_destroy(graph)


@pytest.mark.parametrize("first", ["older", "newer"])
def test_two_live_graphs_with_growth_in_between(first, ckks14, capi):
    """graph 1 at batch 2, growth, graph 2 at batch 8, growth: each holds its own workspace until it is destroyed (arena)"""
    o, _ = ckks14
    g = _context(capi, o, KEY_SEED)
    r1 = Rig(o, g, 2, seed=21)
    g1 = r1.record()
    r2 = Rig(o, g, 8, seed=22)
    g2 = r2.record()  # its eager pass grows the workspace: graph 1's is held back
    assert g.held_buffers() > 0
    big = _random_cts(o, 32, g.L, 13)
    _same("eager mul_relin at batch 32", g.mul_relin(big, big)[31], o.mul_relin(big[31], big[31]))
    held = g.held_buffers()
    assert held >= 2  # one workspace per graph
    r1.set_inputs(23)
    r2.set_inputs(24)
    r1.replay(g1, what="graph 1 with both alive")
    r2.replay(g2, what="graph 2 with both alive")
    order = [(g1, r1, g2, r2), (g2, r2, g1, r1)][first == "newer"]
    gone, _, alive, rig = order
    g.graph_destroy(gone)
    assert 0 < g.held_buffers() < held  # what only the destroyed graph held is freed, the rest stays
    rig.set_inputs(25)
    rig.replay(alive, what="surviving graph")
    g.graph_destroy(alive)
    assert g.held_buffers() == 0
