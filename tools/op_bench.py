"""Per-operation throughput of the C ABI on one MI355X (batched, operands resident in HBM).
Not the bench line (bench.py is); numbers quoted in DESIGN.md / README.md come from here."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from abc_amd import capi


def timeit(g, fn, reps=10):
    fn(); g.sync()
    g.timer_start()
    for _ in range(reps):
        fn()
    return g.timer_stop() / reps


def rand_ct(g, rng, batch, size, nl):
    x = np.stack([rng.integers(0, q, size=(batch, size, g.n), dtype=np.uint64) for q in g.primes[:nl]], axis=2)
    return g.upload(x), x.nbytes


def rotate_add_ab(res, only, rng):
    """addend + rotate(in, 1) as abc_hip_rotate into a temporary followed by abc_hip_add, against one abc_hip_rotate_add: alternating in
    one process, five runs each, so that the spread of the separate runs shows (the bar a fused route has to meet: DESIGN.md section 7)"""
    shapes = [  # tag, context, level or None for L, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), (3, 4), (512, 32)),
        ("ckks15", lambda: capi.Context(capi.CKKS, 32768, capi.create_primes(32768, [50, 40, 40, 50])), (3,), (256, 32)),
        ("bfv16384", lambda: capi.Context.bfv_default(16384), (None,), (256,)),
        ("bfv8192", lambda: capi.Context.bfv_default(8192), (None,), (512,)),
    ]
    for tag, make, levels, batches in shapes:
        if only and only not in "%s_rotate_add" % tag and "rotate_add" not in only:  # no entry of this context can match
            continue
        g = make()
        g.keygen(1)
        for level in levels:
            nl = level or g.L
            for B in batches:
                names = ["%s_L%d_b%d_rotate_add_%s" % (tag, nl, B, kind) for kind in ("separate", "fused")]
                if not any(only in k for k in names):
                    continue
                cb = C.c_size_t(B)
                a, nb = rand_ct(g, rng, B, 2, nl)
                b, _ = rand_ct(g, rng, B, 2, nl)
                tmp, out = g.alloc(nb), g.alloc(nb)

                def separate():
                    g.op("rotate", a.ptr, tmp.ptr, nl, 1, cb)
                    g.op("add", b.ptr, tmp.ptr, out.ptr, 2, nl, cb)

                def fused():
                    g.op("rotate_add", a.ptr, b.ptr, out.ptr, nl, 1, cb)
                runs = {names[0]: [], names[1]: []}
                for rep in range(10):  # separate, fused, separate, fused, ...
                    runs[names[rep & 1]].append(timeit(g, fused if rep & 1 else separate))
                for k, ms in runs.items():
                    route = g.route("rotate_add" if k == names[1] else "rotate", nl, B)
                    res[k] = {"batch": B, "ms": min(ms), "ms_median": sorted(ms)[len(ms) // 2], "ms_runs": ms, "route": route}
                    print("%-44s %s ms / %d  (%s)" % (k, " ".join("%8.3f" % v for v in ms), B, route), flush=True)
                del a, b, tmp, out
        g.close()


def _alternate(g, res, names, fns, routes, B, reps=10):
    """fns[0], fns[1], fns[0], ...: five runs each.  The first run of fns[0] sizes the arenas and is left out of its minimum."""
    runs = {names[0]: [], names[1]: []}
    for rep in range(10):
        runs[names[rep & 1]].append(timeit(g, fns[rep & 1], reps))
    for i, (k, ms) in enumerate(runs.items()):
        kept = ms[1:] if i == 0 else ms
        res[k] = {"batch": B, "ms": min(kept), "ms_median": sorted(kept)[len(kept) // 2], "ms_runs": ms, "route": routes[i]}
        print("%-44s %s ms / %d  (%s)" % (k, " ".join("%8.3f" % v for v in ms), B, routes[i]), flush=True)


def rotate_mac_ab(res, only, rng):
    """addend + plain (.) rotate(in, 1) as abc_hip_rotate into a temporary, abc_hip_multiply_plain on it and abc_hip_add, against one
    abc_hip_rotate_mac_plain; and an eight-diagonal abc_hip_diag_matvec against eight such triples (the first without its add).  Alternating in one process, five
    runs each; a shape stays on the fused route only if every fused run beats the fastest separate one."""
    shapes = [  # tag, context, levels, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), (3, 4), (512, 32)),
        ("ckks15", lambda: capi.Context(capi.CKKS, 32768, capi.create_primes(32768, [50, 40, 40, 50])), (3,), (256, 32)),
    ]
    for tag, make, levels, batches in shapes:
        if only and only not in "%s_rotate_mac" % tag and "rotate_mac" not in only:  # no entry of this context can match
            continue
        g = make()
        g.keygen(1)
        for nl in levels:
            for B in batches:
                names = ["%s_L%d_b%d_rotate_mac_%s" % (tag, nl, B, kind) for kind in ("separate", "fused")]
                if not any(only in k for k in names):
                    continue
                cb, zero = C.c_size_t(B), C.c_size_t(0)
                a, nb = rand_ct(g, rng, B, 2, nl)
                b, _ = rand_ct(g, rng, B, 2, nl)
                p, _ = rand_ct(g, rng, 1, 1, nl)  # one plaintext [nl][N], broadcast
                tmp, out = g.alloc(nb), g.alloc(nb)

                def separate():
                    g.op("rotate", a.ptr, tmp.ptr, nl, 1, cb)
                    g.op("multiply_plain", tmp.ptr, p.ptr, zero, tmp.ptr, 2, nl, cb)
                    g.op("add", b.ptr, tmp.ptr, out.ptr, 2, nl, cb)

                def fused():
                    g.op("rotate_mac_plain", a.ptr, p.ptr, zero, b.ptr, out.ptr, nl, 1, cb)
                _alternate(g, res, names, (separate, fused), (g.route("rotate", nl, B), g.route("rotate_mac_plain", nl, B)), B)
                del a, b, p, tmp, out
        names = ["%s_L3_b512_rotate_mac_diag8_%s" % (tag, kind) for kind in ("separate", "fused")]
        if tag == "ckks14" and any(only in k for k in names):
            nl, B, H = 3, 512, 8
            steps = [1 << i for i in range(H)]
            cb, zero = C.c_size_t(B), C.c_size_t(0)
            a, nb = rand_ct(g, rng, B, 2, nl)
            d, db = rand_ct(g, rng, H, 1, nl)  # [H][nl][N]
            row = [C.c_void_p(d.ptr.value + r * (db // H)) for r in range(H)]
            tmp, out = g.alloc(nb), g.alloc(nb)
            arr = (C.c_int * H)(*steps)

            def separate():
                for r in range(H):
                    dst = tmp if r else out
                    g.op("rotate", a.ptr, dst.ptr, nl, steps[r], cb)
                    g.op("multiply_plain", dst.ptr, row[r], zero, dst.ptr, 2, nl, cb)
                    if r:
                        g.op("add", out.ptr, tmp.ptr, out.ptr, 2, nl, cb)

            def fused():
                g.op("diag_matvec", a.ptr, d.ptr, C.c_size_t(nl * g.n), arr, H, out.ptr, nl, cb)
            _alternate(g, res, names, (separate, fused), (g.route("rotate", nl, B), g.route("rotate_mac_plain", nl, B)), B)
            del a, d, tmp, out
        g.close()


def mulplain_rescale_ab(res, only, rng):
    """rescale(ct (.) plain), one plaintext for the batch, as abc_hip_multiply_plain into a temporary followed by abc_hip_rescale, against
    one abc_hip_multiply_plain_rescale.  Alternating in one process, five runs each; a shape stays on the fused route only if its fused
    median is not above its separate median."""
    shapes = [  # tag, context, levels, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), (4, 3), (512, 32)),
        ("ckks12", lambda: capi.Context(capi.CKKS, 4096, capi.create_primes(4096, [50, 40, 40, 50])), (3,), (1024,)),
    ]
    for tag, make, levels, batches in shapes:
        if only and only not in "%s_mulplain_rescale" % tag and "mulplain_rescale" not in only:  # no entry of this context can match
            continue
        g = make()
        for nl in levels:
            for B in batches:
                names = ["%s_L%d_b%d_mulplain_rescale_%s" % (tag, nl, B, kind) for kind in ("separate", "fused")]
                if not any(only in k for k in names):
                    continue
                cb, zero = C.c_size_t(B), C.c_size_t(0)
                a, nb = rand_ct(g, rng, B, 2, nl)
                p, _ = rand_ct(g, rng, 1, 1, nl)  # one plaintext [nl][N], broadcast
                tmp, out = g.alloc(nb), g.alloc(nb // nl * (nl - 1))

                def separate():
                    g.op("multiply_plain", a.ptr, p.ptr, zero, tmp.ptr, 2, nl, cb)
                    g.op("rescale", tmp.ptr, out.ptr, 2, nl, cb)

                def fused():
                    g.op("multiply_plain_rescale", a.ptr, p.ptr, zero, out.ptr, 2, nl, cb)
                _alternate(g, res, names, (separate, fused), (g.route("rescale", nl, B), g.route("multiply_plain_rescale", nl, B)), B,
                           reps=200)  # calls of 0.04 .. 0.7 ms: a run is 8 .. 140 ms of device time
                del a, p, tmp, out
        g.close()


def mul_sum_ab(res, only, rng):
    """relinearize(sum of K ciphertext products), three ways, alternating in one process, five runs each:
    (a) `eager`: K x abc_hip_mul_relin and K - 1 x abc_hip_add -- what a caller had before the call existed;
    (b) `per_term`: abc_hip_mul_sum_relin under ABC_HIP_NO_TENSOR_SUM=1 (tensor per term, add kernel, one key switch);
    (c) `sum`: abc_hip_mul_sum_relin, the K-term tensor-sum kernel and one key switch (CKKS; BFV has (a) and (b) only).
    The 2 K operands are distinct buffers (device copies of one random batch: the kernels have no data-dependent path)."""
    shapes = [  # tag, context, levels (None: L), batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), (3, 4), (512, 32)),
        ("ckks15", lambda: capi.Context(capi.CKKS, 32768, capi.create_primes(32768, [50, 40, 40, 50])), (3,), (256,)),
        ("ckks12", lambda: capi.Context(capi.CKKS, 4096, capi.create_primes(4096, [50, 40, 40, 50])), (3,), (1024,)),
        ("bfv16384", lambda: capi.Context.bfv_default(16384), (None,), (64,)),
    ]
    switch = "ABC_HIP_NO_TENSOR_SUM"
    for tag, make, levels, batches in shapes:
        if only and only not in "%s_mul_sum" % tag and "mul_sum" not in only:
            continue
        g = make()
        g.keygen(1)
        ckks = g.scheme == capi.CKKS
        kinds = ("eager", "per_term", "sum") if ckks else ("eager", "per_term")
        for level in levels:
            nl = level or g.L
            for B in batches:
                cb = C.c_size_t(B)
                first, nb = rand_ct(g, rng, B, 2, nl)
                pool = [first]
                for _ in range(2 * 16 - 1):
                    pool.append(g.alloc(nb))
                    g.op("memcpy_d2d", pool[-1].ptr, first.ptr, C.c_size_t(nb))
                tmp, out = g.alloc(nb), g.alloc(nb)
                for K in (2, 4, 8, 16):
                    names = ["%s_L%d_b%d_mul_sum_K%d_%s" % (tag, nl, B, K, kind) for kind in kinds]
                    if not any(only in k for k in names):
                        continue
                    pa, pb = g.term_pointers([x.ptr for x in pool[:K]]), g.term_pointers([x.ptr for x in pool[16:16 + K]])

                    def eager():
                        g.op("mul_relin", pool[0].ptr, pool[16].ptr, out.ptr, nl, cb)
                        for k in range(1, K):
                            g.op("mul_relin", pool[k].ptr, pool[16 + k].ptr, tmp.ptr, nl, cb)
                            g.op("add", out.ptr, tmp.ptr, out.ptr, 2, nl, cb)

                    def one_call():
                        g.op("mul_sum_relin", pa, pb, K, out.ptr, nl, cb)
                    runs, routes = {k: [] for k in names}, {}
                    reps = 10 if B * K >= 256 else 50
                    for rep in range(5):
                        for kind, name in zip(kinds, names):
                            if kind == "per_term":
                                os.environ[switch] = "1"
                            else:
                                os.environ.pop(switch, None)
                            g.reload_env()
                            routes[name] = g.route("mul_relin" if kind == "eager" else "mul_sum_relin", nl, B)
                            runs[name].append(timeit(g, eager if kind == "eager" else one_call, reps))
                    os.environ.pop(switch, None)
                    g.reload_env()
                    for k, ms in runs.items():
                        kept = ms[1:]  # the first run of each sizes its arenas
                        res[k] = {"batch": B, "terms": K, "ms": min(kept), "ms_median": sorted(kept)[len(kept) // 2], "ms_runs": ms,
                                  "us_per_ct": min(kept) * 1e3 / B, "route": routes[k]}
                        print("%-44s %s ms / %d  (%s)" % (k, " ".join("%8.3f" % v for v in ms), B, routes[k]), flush=True)
                del pool, first, tmp, out
        g.close()


def _three_ways(g, res, names, kinds, fns, routes, switch, B, reps, extra=None):
    """the variants in turn, five rounds; kind "per_term" runs under `switch`.  The first run of each sizes its arenas and is left out."""
    runs, route = {k: [] for k in names}, {}
    for rep in range(5):
        for kind, name, fn in zip(kinds, names, fns):
            if kind == "per_term":
                os.environ[switch] = "1"
            else:
                os.environ.pop(switch, None)
            g.reload_env()
            route[name] = routes(kind)
            runs[name].append(timeit(g, fn, reps))
    os.environ.pop(switch, None)
    g.reload_env()
    for i, (k, ms) in enumerate(runs.items()):
        kept = ms[1:]
        res[k] = {"batch": B, "ms": min(kept), "ms_median": sorted(kept)[len(kept) // 2], "ms_runs": ms, "us_per_ct": min(kept) * 1e3 / B,
                  "route": route[k]}
        res[k].update(extra[i] if extra else {})
        note = "  [%s]" % ", ".join("%s %s" % kv for kv in extra[i].items()) if extra else ""
        print("%-48s %s ms / %d  (%s)%s" % (k, " ".join("%8.3f" % v for v in ms), B, route[k], note), flush=True)


def plain_mac_sum_ab(res, only, rng):
    """sum over K terms of plain_k (.) ct_k, one plaintext per term for the batch, three ways, alternating in one process, five runs each:
    (a) `composed`: K x abc_hip_multiply_plain and K - 1 x abc_hip_add -- what a caller had before the call existed;
    (b) `per_term`: abc_hip_multiply_plain_sum under ABC_HIP_NO_PLAIN_MAC_SUM=1;
    (c) `kernel`: abc_hip_multiply_plain_sum, the K-term kernel.
    The K ciphertext operands are distinct buffers (device copies of one random batch: the kernels have no data-dependent path)."""
    shapes = [  # tag, context, levels, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), (4, 3), (512, 32)),
        ("ckks15", lambda: capi.Context(capi.CKKS, 32768, capi.create_primes(32768, [50, 40, 40, 50])), (3,), (256,)),
        ("ckks12", lambda: capi.Context(capi.CKKS, 4096, capi.create_primes(4096, [50, 40, 40, 50])), (3,), (1024,)),
    ]
    kinds = ("composed", "per_term", "kernel")
    for tag, make, levels, batches in shapes:
        if only and only not in "%s_plain_mac_sum" % tag and "plain_mac_sum" not in only:
            continue
        g = make()
        for nl in levels:
            for B in batches:
                cb, zero = C.c_size_t(B), C.c_size_t(0)
                first, nb = rand_ct(g, rng, B, 2, nl)
                pool = [first]
                for _ in range(15):
                    pool.append(g.alloc(nb))
                    g.op("memcpy_d2d", pool[-1].ptr, first.ptr, C.c_size_t(nb))
                plains = [rand_ct(g, rng, 1, 1, nl)[0] for _ in range(16)]  # [nl][N] each
                tmp, out = g.alloc(nb), g.alloc(nb)
                for K in (2, 4, 8, 16):
                    names = ["%s_L%d_b%d_plain_mac_sum_K%d_%s" % (tag, nl, B, K, kind) for kind in kinds]
                    if not any(only in k for k in names):
                        continue
                    pc, pp = g.term_pointers([x.ptr for x in pool[:K]]), g.term_pointers([x.ptr for x in plains[:K]])

                    def composed():
                        g.op("multiply_plain", pool[0].ptr, plains[0].ptr, zero, out.ptr, 2, nl, cb)
                        for k in range(1, K):
                            g.op("multiply_plain", pool[k].ptr, plains[k].ptr, zero, tmp.ptr, 2, nl, cb)
                            g.op("add", out.ptr, tmp.ptr, out.ptr, 2, nl, cb)

                    def one_call():
                        g.op("multiply_plain_sum", pc, pp, zero, K, None, out.ptr, 2, nl, cb)
                    _three_ways(g, res, names, kinds, (composed, one_call, one_call),
                                lambda kind: "composed" if kind == "composed" else g.route("diag_matvec_bsgs", nl, B).split(" add=")[0].split(" ")[-1],
                                "ABC_HIP_NO_PLAIN_MAC_SUM", B, 10 if B * K >= 256 else 50)
                del pool, first, plains, tmp, out
        g.close()


def _naf(value):
    out, sign, value, i = [], value < 0, abs(value), 0
    while value:
        zi = 2 - (value & 3) if value & 1 else 0
        value = (value - zi) >> 1
        if zi:
            out.append((-zi if sign else zi) << i)
        i += 1
    return out


def _key_switches(g, steps):
    """key switches abc_hip_rotate performs for these steps under the context's key set: one with a key of its own, else the NAF chain's"""
    have = set(g.galois_elts())
    return sum(0 if s == 0 else 1 if g.elt_from_step(s) in have else len(_naf(s)) for s in steps)


def matvec_bsgs_ab(res, only, rng):
    """a matrix of n diagonals (steps 0 .. n - 1) times a batch of ciphertexts: abc_hip_diag_matvec, one rotation per diagonal, against
    abc_hip_diag_matvec_bsgs on the same diagonals as a square grid (16 = 4 x 4, 64 = 8 x 8), alternating in one process, five runs
    each.  The default key set on both sides, so both pay NAF chains; the number of key switches of each side is printed with its time."""
    shapes = [  # tag, context, level, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), 3, (512, 32)),
        ("ckks15", lambda: capi.Context(capi.CKKS, 32768, capi.create_primes(32768, [50, 40, 40, 50])), 3, (256,)),
    ]
    kinds = ("diag_matvec", "bsgs")
    for tag, make, nl, batches in shapes:
        if only and only not in "%s_matvec_bsgs" % tag and "matvec_bsgs" not in only:
            continue
        g = make()
        g.keygen(1)
        for B in batches:
            cb = C.c_size_t(B)
            a, nb = rand_ct(g, rng, B, 2, nl)
            d, _ = rand_ct(g, rng, 64, 1, nl)  # [64][nl][N]: the words do not matter to the time, so one set serves both sides
            out = g.alloc(nb)
            for side in (4, 8):
                n = side * side
                names = ["%s_L%d_b%d_matvec_bsgs_%dx%d_%s" % (tag, nl, B, side, side, kind) for kind in kinds]
                if not any(only in k for k in names):
                    continue
                steps, baby, giant = list(range(n)), list(range(side)), [side * j for j in range(side)]
                c_steps, c_baby, c_giant = (C.c_int * n)(*steps), (C.c_int * side)(*baby), (C.c_int * side)(*giant)
                stride = C.c_size_t(nl * g.n)

                def diag():
                    g.op("diag_matvec", a.ptr, d.ptr, stride, c_steps, n, out.ptr, nl, cb)

                def bsgs():
                    g.op("diag_matvec_bsgs", a.ptr, d.ptr, stride, c_baby, side, c_giant, side, out.ptr, nl, cb)
                extra = ({"key_switches": _key_switches(g, steps)}, {"key_switches": _key_switches(g, baby) + _key_switches(g, giant)})
                _three_ways(g, res, names, kinds, (diag, bsgs),
                            lambda kind: g.route("rotate_mac_plain" if kind == "diag_matvec" else "diag_matvec_bsgs", nl, B), "ABC_HIP_NO_PLAIN_MAC_SUM",
                            B, 3, extra)
                t_d, t_b = res[names[0]]["ms_median"], res[names[1]]["ms_median"]
                print("    time ratio %.2f, key-switch ratio %.2f" % (t_d / t_b, extra[0]["key_switches"] / extra[1]["key_switches"]), flush=True)
            del a, d, out
        g.close()


def _env_rounds(g, res, names, fns, envs, route_op, nl, B, reps, extra=None):
    """the variants in turn, five rounds, variant i under the environment envs[i] (read by reload_env, cleared afterwards).  The first run
    of each sizes its arenas and is left out of its minimum and median."""
    runs, route = {k: [] for k in names}, {}
    keys = sorted({k for e in envs for k in e})
    for _ in range(5):
        for name, fn, env in zip(names, fns, envs):
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(env)
            g.reload_env()
            route[name] = g.route(route_op, nl, B)
            runs[name].append(timeit(g, fn, reps))
    for k in keys:
        os.environ.pop(k, None)
    g.reload_env()
    for i, (k, ms) in enumerate(runs.items()):
        kept = ms[1:]
        res[k] = {"batch": B, "ms": min(kept), "ms_median": sorted(kept)[len(kept) // 2], "ms_spread": max(kept) - min(kept), "ms_runs": ms,
                  "us_per_ct": min(kept) * 1e3 / B, "route": route[k], "env": envs[i]}
        res[k].update(extra[i] if extra else {})
        note = "  [%s]" % ", ".join("%s %s" % kv for kv in extra[i].items()) if extra else ""
        print("%-50s %s ms / %d  (%s)%s" % (k, " ".join("%8.3f" % v for v in ms), B, route[k], note), flush=True)


def plain_sum_rescale_ab(res, only, rng):
    """rescale(sum over K terms of plain_k (.) ct_k), one plaintext per term for the batch, alternating in one process, five runs each:
    (a) `two_calls`: abc_hip_multiply_plain_sum into a temporary, then abc_hip_rescale -- what a caller had before the call existed;
    (b) `separate`: abc_hip_multiply_plain_sum_rescale under ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION=1;
    (c) `default`: the call as the route sends it (abc_route.hpp, route_plain_sum_rescale: the rule these numbers gave);
    (d) `fused8` / `fused4` / `fused2` / `fused0`: the call with the fused pair at every shape, taking at most that many terms
        (ABC_HIP_PLAIN_SUM_RESCALE_TERMS; 0: the carry alone), the streaming kernel the ones before."""
    shapes = [  # tag, context, levels, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), (4, 3), (512, 128, 64, 32)),
        ("ckks12", lambda: capi.Context(capi.CKKS, 4096, capi.create_primes(4096, [50, 40, 40, 50])), (3,), (1024, 128, 64)),
        ("ckks10", lambda: capi.Context(capi.CKKS, 1024, capi.create_primes(1024, [50, 40, 40, 50])), (3,), (1024, 256)),
    ]
    fused = (8, 4, 2, 0)
    kinds = ("two_calls", "separate", "default") + tuple("fused%d" % f for f in fused)
    envs = ({}, {"ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION": "1"}, {}) + tuple({"ABC_HIP_PLAIN_SUM_RESCALE_TERMS": str(f)} for f in fused)
    for tag, make, levels, batches in shapes:
        if only and only not in "%s_plain_sum_rescale" % tag and "plain_sum_rescale" not in only:
            continue
        g = make()
        for nl in levels:
            for B in batches:
                cb, zero = C.c_size_t(B), C.c_size_t(0)
                first, nb = rand_ct(g, rng, B, 2, nl)
                pool = [first]
                for _ in range(15):
                    pool.append(g.alloc(nb))
                    g.op("memcpy_d2d", pool[-1].ptr, first.ptr, C.c_size_t(nb))
                plains = [rand_ct(g, rng, 1, 1, nl)[0] for _ in range(16)]  # [nl][N] each
                tmp, out = g.alloc(nb), g.alloc(nb)
                for K in (1, 2, 3, 4, 6, 8, 16):
                    names = ["%s_L%d_b%d_plain_sum_rescale_K%d_%s" % (tag, nl, B, K, kind) for kind in kinds]
                    if not any(only in k for k in names):
                        continue
                    pc, pp = g.term_pointers([x.ptr for x in pool[:K]]), g.term_pointers([x.ptr for x in plains[:K]])

                    def two_calls():
                        g.op("multiply_plain_sum", pc, pp, zero, K, None, tmp.ptr, 2, nl, cb)
                        g.op("rescale", tmp.ptr, out.ptr, 2, nl, cb)

                    def one_call():
                        g.op("multiply_plain_sum_rescale", pc, pp, zero, K, None, out.ptr, 2, nl, cb)
                    _env_rounds(g, res, names, (two_calls,) + (one_call,) * (len(kinds) - 1), envs, "plain_sum_rescale", nl, B, 10 if B * K >= 256 else 50)
                    base = res[names[0]]
                    print("    two calls / variant: " + ", ".join("%s %.2f" % (kind, base["ms_median"] / res[k]["ms_median"]) for kind, k in zip(kinds[1:], names[1:])) +
                          "   (spread of the two calls: %.3f ms)" % base["ms_spread"], flush=True)
                del pool, first, plains, tmp, out
        g.close()


def matvec_bsgs_rescale_ab(res, only, rng):
    """rescale(abc_hip_diag_matvec_bsgs(...)) against abc_hip_diag_matvec_bsgs_rescale on the same pre-rotated rows, as a square grid (16 =
    4 x 4, 64 = 8 x 8), alternating in one process, five runs each; the default key set, so both pay the same NAF chains.  Printed with
    each time: the key switches and the limb count they run at (baby steps at nl on both sides; giant steps at nl against nl - 1)."""
    shapes = [  # tag, context, level, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), 3, (512, 32)),
        ("ckks15", lambda: capi.Context(capi.CKKS, 32768, capi.create_primes(32768, [50, 40, 40, 50])), 3, (256,)),
    ]
    kinds = ("rescale_after", "rescale_before")
    for tag, make, nl, batches in shapes:
        if only and only not in "%s_matvec_bsgs_rescale" % tag and "matvec_bsgs_rescale" not in only:
            continue
        g = make()
        g.keygen(1)
        for B in batches:
            cb = C.c_size_t(B)
            a, nb = rand_ct(g, rng, B, 2, nl)
            d, _ = rand_ct(g, rng, 64, 1, nl)  # [64][nl][N]: the words do not matter to the time
            tmp, out = g.alloc(nb), g.alloc(nb)
            for side in (4, 8):
                names = ["%s_L%d_b%d_matvec_bsgs_rescale_%dx%d_%s" % (tag, nl, B, side, side, kind) for kind in kinds]
                if not any(only in k for k in names):
                    continue
                baby, giant = list(range(side)), [side * j for j in range(side)]
                c_baby, c_giant = (C.c_int * side)(*baby), (C.c_int * side)(*giant)
                stride = C.c_size_t(nl * g.n)

                def after():
                    g.op("diag_matvec_bsgs", a.ptr, d.ptr, stride, c_baby, side, c_giant, side, tmp.ptr, nl, cb)
                    g.op("rescale", tmp.ptr, out.ptr, 2, nl, cb)

                def before():
                    g.op("diag_matvec_bsgs_rescale", a.ptr, d.ptr, stride, c_baby, side, c_giant, side, out.ptr, nl, cb)
                kb, kg = _key_switches(g, baby), _key_switches(g, giant)
                extra = ({"key_switches": "%d at %d limbs + %d at %d" % (kb, nl, kg, nl), "rescales": 1},
                         {"key_switches": "%d at %d limbs + %d at %d" % (kb, nl, kg, nl - 1), "rescales": side})
                _env_rounds(g, res, names, (after, before), ({}, {}), "diag_matvec_bsgs_rescale", nl, B, 3, extra)
                res[names[0]]["route"] = g.route("diag_matvec_bsgs", nl, B) + ", then " + g.route("rescale", nl, B)
                print("    rescale after / rescale before: %.2f   (spread of rescale after: %.3f ms)" %
                      (res[names[0]]["ms_median"] / res[names[1]]["ms_median"], res[names[0]]["ms_spread"]), flush=True)
            del a, d, tmp, out
        g.close()


def _rounds(g, res, names, fns, routes, B, reps, extra=None):
    """fns[0], fns[1], ..., fns[0], ...: five runs each in one process.  The first run of EVERY variant sizes its arenas and is left
    out of its minimum, median and ratio (it is still printed, first in its row)."""
    runs = {k: [] for k in names}
    for _ in range(5):
        for k, fn in zip(names, fns):
            runs[k].append(timeit(g, fn, reps))
    for i, (k, ms) in enumerate(runs.items()):
        kept = ms[1:]
        res[k] = {"batch": B, "ms": min(kept), "ms_median": sorted(kept)[len(kept) // 2], "ms_runs": ms, "route": routes[i]}
        res[k].update(extra[i] if extra else {})
        print("%-52s %s ms / %d  (%s)%s" % (k, " ".join("%8.3f" % v for v in ms), B, routes[i], "  %s" % extra[i] if extra else ""), flush=True)
    base = res[names[0]]["ms_median"]
    print("    composed / new call: " + ", ".join("%.2f" % (base / res[k]["ms_median"]) for k in names[1:]), flush=True)


def bfv_plain_sum_ab(res, only, rng):
    """BFV: sum over K terms of plain_k * ct_k, one plaintext per term for the batch, alternating in one process, five runs each:
    (a) `composed`: K x abc_hip_multiply_plain (plaintexts modulo t: lifted and transformed on every call) and K - 1 x abc_hip_add;
    (b) `sum_coeff`: abc_hip_bfv_multiply_plain_sum on coefficient-form terms, plaintexts transformed once beforehand;
    (c) `sum_ntt`: the same call on terms already in NTT form (the inner sum of the matvec)."""
    def chain15():
        n = 32768
        return capi.Context(capi.BFV, n, capi.create_primes(n, [55] * 16), capi.plain_modulus_batching(n, 20))
    shapes = [("bfv16384", lambda: capi.Context.bfv_default(16384), 256), ("bfv8192", lambda: capi.Context.bfv_default(8192), 512),
              ("bfv4096", lambda: capi.Context.bfv_default(4096), 1024), ("bfv32768x15", chain15, 64)]
    kinds = ("composed", "sum_coeff", "sum_ntt")
    for tag, make, B in shapes:
        if only and only not in "%s_bfv_plain_sum" % tag and "bfv_plain_sum" not in only:
            continue
        g = make()
        L, cb, zero = g.L, C.c_size_t(B), C.c_size_t(0)
        first, nb = rand_ct(g, rng, B, 2, L)
        pool = [first]
        for _ in range(15):
            pool.append(g.alloc(nb))
            g.op("memcpy_d2d", pool[-1].ptr, first.ptr, C.c_size_t(nb))
        plains = g.upload(rng.integers(0, g.t, size=(16, g.n), dtype=np.uint64))
        plains_ntt = g.alloc(16 * L * g.n * 8)
        g.op("bfv_plain_to_ntt", plains.ptr, plains_ntt.ptr, C.c_size_t(16))
        tmp, out = g.alloc(nb), g.alloc(nb)
        for K in (2, 4, 8, 16):
            names = ["%s_b%d_bfv_plain_sum_K%d_%s" % (tag, B, K, kind) for kind in kinds]
            if not any(only in k for k in names):
                continue
            pm = [C.c_void_p(plains.ptr.value + 8 * k * g.n) for k in range(K)]
            pc = g.term_pointers([x.ptr for x in pool[:K]])
            pp = g.term_pointers([C.c_void_p(plains_ntt.ptr.value + 8 * k * L * g.n) for k in range(K)])

            def composed():
                g.op("multiply_plain", pool[0].ptr, pm[0], zero, out.ptr, 2, L, cb)
                for k in range(1, K):
                    g.op("multiply_plain", pool[k].ptr, pm[k], zero, tmp.ptr, 2, L, cb)
                    g.op("add", out.ptr, tmp.ptr, out.ptr, 2, L, cb)

            def sum_coeff():
                g.op("bfv_multiply_plain_sum", pc, 0, pp, zero, K, None, out.ptr, 2, cb)

            def sum_ntt():
                g.op("bfv_multiply_plain_sum", pc, 1, pp, zero, K, None, out.ptr, 2, cb)
            route = g.route("bfv_plain_sum", L, B)
            _rounds(g, res, names, (composed, sum_coeff, sum_ntt), ("composed", route, route), B, 5)
        del pool, first, plains, plains_ntt, tmp, out
        g.close()


def bfv_matvec_bsgs_ab(res, only, rng):
    """BFV: a matrix of n diagonals times a batch of ciphertexts: n x (abc_hip_rotate, abc_hip_multiply_plain, abc_hip_add) against
    abc_hip_bfv_diag_matvec_bsgs on a square grid (16 = 4 x 4, 64 = 8 x 8), alternating in one process, five runs each.  The default
    key set on both sides, so both pay NAF chains; the key switches of each side are printed with its time."""
    shapes = [("bfv16384", lambda: capi.Context.bfv_default(16384), 256), ("bfv8192", lambda: capi.Context.bfv_default(8192), 512)]
    kinds = ("composed", "bsgs")
    for tag, make, B in shapes:
        if only and only not in "%s_bfv_matvec_bsgs" % tag and "bfv_matvec_bsgs" not in only:
            continue
        g = make()
        g.keygen(1)
        L, cb, zero = g.L, C.c_size_t(B), C.c_size_t(0)
        a, nb = rand_ct(g, rng, B, 2, L)
        plains = g.upload(rng.integers(0, g.t, size=(64, g.n), dtype=np.uint64))
        d = g.alloc(64 * L * g.n * 8)
        g.op("bfv_plain_to_ntt", plains.ptr, d.ptr, C.c_size_t(64))
        rot, tmp, out = g.alloc(nb), g.alloc(nb), g.alloc(nb)
        for side in (4, 8):
            n = side * side
            names = ["%s_b%d_bfv_matvec_bsgs_%dx%d_%s" % (tag, B, side, side, kind) for kind in kinds]
            if not any(only in k for k in names):
                continue
            steps, baby, giant = list(range(n)), list(range(side)), [side * j for j in range(side)]
            c_baby, c_giant = (C.c_int * side)(*baby), (C.c_int * side)(*giant)
            pm = [C.c_void_p(plains.ptr.value + 8 * k * g.n) for k in range(n)]

            def composed():
                g.op("multiply_plain", a.ptr, pm[0], zero, out.ptr, 2, L, cb)
                for s in steps[1:]:
                    g.op("rotate", a.ptr, rot.ptr, L, s, cb)
                    g.op("multiply_plain", rot.ptr, pm[s], zero, tmp.ptr, 2, L, cb)
                    g.op("add", out.ptr, tmp.ptr, out.ptr, 2, L, cb)

            def bsgs():
                g.op("bfv_diag_matvec_bsgs", a.ptr, d.ptr, C.c_size_t(L * g.n), c_baby, side, c_giant, side, out.ptr, cb)
            extra = ({"key_switches": _key_switches(g, steps)}, {"key_switches": _key_switches(g, baby) + _key_switches(g, giant)})
            _rounds(g, res, names, (composed, bsgs), (g.route("rotate", L, B), g.route("bfv_matvec_bsgs", L, B)), B, 2, extra)
        del a, plains, d, rot, tmp, out
        g.close()


def keyswitch_batch1(res, only, rng):
    """one ciphertext per call at nl = 4: relinearise, rotate, rotate_add and rotate_mac_plain (one plaintext, one addend) on the two
    CKKS split rings -- the calls in which the host side of the key switch (routes, operand record, launches) is the largest share"""
    for n in (16384, 32768):
        names = ["ckks%d_b1_%s" % (n.bit_length() - 1, op) for op in ("relinearize", "rotate", "rotate_add", "rotate_mac_plain")]
        if not any(only in k for k in names):
            continue
        g = capi.Context(capi.CKKS, n, capi.create_primes(n, [50, 40, 40, 40, 50]))
        g.keygen(1)
        one, zero = C.c_size_t(1), C.c_size_t(0)
        (a, nb), (b, _), (t3, _), (p, _) = rand_ct(g, rng, 1, 2, 4), rand_ct(g, rng, 1, 2, 4), rand_ct(g, rng, 1, 3, 4), rand_ct(g, rng, 1, 1, 4)
        out = g.alloc(nb)
        ops = [lambda: g.op("relinearize", t3.ptr, out.ptr, 4, one), lambda: g.op("rotate", a.ptr, out.ptr, 4, 1, one),
               lambda: g.op("rotate_add", a.ptr, b.ptr, out.ptr, 4, 1, one)]
        if hasattr(capi.lib(), "abc_hip_rotate_mac_plain"):  # not in a build older than the call (ABC_HIP_LIB)
            ops.append(lambda: g.op("rotate_mac_plain", a.ptr, p.ptr, zero, b.ptr, out.ptr, 4, 1, one))
        for k, fn in zip(names, ops):
            if only in k:
                timeit(g, fn, reps=20)
                ms = timeit(g, fn, reps=300)
                res[k] = {"batch": 1, "ms": ms, "route": g.route(k.split("_b1_")[1], 4, 1)}
                print("%-40s %8.3f us (batch 1; %s)" % (k, ms * 1e3, res[k]["route"]), flush=True)
        del a, b, t3, p, out
        g.close()


def single_ops(res, only, rng):
    """the single operations: every context of this part is created whatever --only says"""
    # ---- CKKS N=2^14, 4 limbs ----
    n, B = 16384, 512
    g = capi.Context(capi.CKKS, n, capi.create_primes(n, [50, 40, 40, 40, 50]))
    g.keygen(1)
    a, nb = rand_ct(g, rng, B, 2, 4)
    b, _ = rand_ct(g, rng, B, 2, 4)
    out = g.alloc(nb)
    cb = C.c_size_t(B)
    ops = {
        "ckks14_mul_relin": lambda: g.op("mul_relin", a.ptr, b.ptr, out.ptr, 4, cb),
        "ckks14_rotate_1": lambda: g.op("rotate", a.ptr, out.ptr, 4, 1, cb),
        "ckks14_rotate_3(NAF:2 key switches)": lambda: g.op("rotate", a.ptr, out.ptr, 4, 3, cb),
        "ckks14_add": lambda: g.op("add", a.ptr, b.ptr, out.ptr, 2, 4, cb),
        "ckks14_rescale": lambda: g.op("rescale", a.ptr, out.ptr, 2, 4, cb),
    }
    for k, fn in ops.items():
        if only not in k:
            continue
        ms = timeit(g, fn)
        res[k] = {"batch": B, "ms": ms, "ops_per_s": B / ms * 1e3}
        print("%-40s %8.3f ms / %d  -> %10.0f op/s" % (k, ms, B, B / ms * 1e3), flush=True)
    del a, b, out
    # ---- H rotations of one input at nl = 3 (the level of config 3's rotations): H abc_hip_rotate calls against one
    # abc_hip_rotate_hoisted call, alternating in one process, the separate calls repeated so that their own spread shows ----
    for H in (2, 8):
        names = ["ckks14_L3_rotate_x%d_%s" % (H, kind) for kind in ("separate", "hoisted")]
        if not any(only in k for k in names):
            continue
        steps = [1 << i for i in range(H)]
        a, nb = rand_ct(g, rng, B, 2, 3)
        outs = g.alloc(H * nb)
        slab = [C.c_void_p(outs.ptr.value + r * nb) for r in range(H)]
        arr = (C.c_int * H)(*steps)

        def separate():
            for r in range(H):
                g.op("rotate", a.ptr, slab[r], 3, steps[r], cb)
        runs = {names[0]: [], names[1]: []}
        for rep in range(5):  # separate, hoisted, separate, hoisted, separate
            k = names[rep & 1]
            if only in k:
                runs[k].append(timeit(g, separate if not rep & 1 else lambda: g.op("rotate_hoisted", a.ptr, outs.ptr, 3, arr, H, cb)))
        for k, ms in runs.items():
            if ms:
                res[k] = {"batch": B, "rotations": H, "ms": min(ms), "ms_runs": ms, "route": g.route("keyswitch" if k == names[1] else "rotate", 3, B)}
                print("%-40s %s ms / %d x %d  (%s)" % (k, " ".join("%8.3f" % v for v in ms), H, B, res[k]["route"]), flush=True)
        del a, outs
    g.close()
    # ---- CKKS slot codec (abc_hip_ckks_encode / _decode), batch 256; bytes = the minimum HBM traffic of the sequence ----
    hbm = 8e12  # MI355X HBM3E peak, bytes/s
    for n, bits in ((16384, [50, 40, 40, 40, 50]), (65536, [60] + [50] * 7 + [60])):
        g = capi.Context(capi.CKKS, n, capi.create_primes(n, bits))
        nl, B, slots = len(bits) - 1, 256, n // 2
        vals = g.upload(rng.uniform(-1, 1, (B, slots)))
        plain, re, im = g.alloc(B * nl * n * 8), g.alloc(B * slots * 8), g.alloc(B * slots * 8)
        cb = C.c_size_t(B)
        words = nl * n * 8
        for name, fn, nbytes in (
            # encode: slot values in, residues out, forward NTT reads and writes them again
            ("ckks%d_encode_L%d" % (n.bit_length() - 1, nl),
             lambda: g.op("ckks_encode", vals.ptr, None, C.c_size_t(slots), C.c_double(2.0 ** 40), nl, plain.ptr, cb),
             slots * 8 + 3 * words),
            # decode: copy to scratch (read + write), inverse NTT (read + write), lift (read), real + imaginary slots out
            ("ckks%d_decode_L%d" % (n.bit_length() - 1, nl),
             lambda: g.op("ckks_decode", plain.ptr, nl, C.c_double(2.0 ** 40), re.ptr, im.ptr, cb),
             5 * words + 2 * slots * 8)):
            if only not in name:
                continue
            ms = timeit(g, fn)
            gbs = B * nbytes / ms * 1e-6
            res[name] = {"batch": B, "ms": ms, "ops_per_s": B / ms * 1e3, "GB_per_s": gbs, "hbm_fraction": gbs * 1e9 / hbm}
            print("%-40s %8.3f ms / %d  -> %10.0f op/s  %7.0f GB/s (%.0f %% of HBM)" % (name, ms, B, B / ms * 1e3, gbs, 100 * gbs * 1e9 / hbm),
                  flush=True)
        del vals, plain, re, im
        g.close()
    # ---- BFV N=2^12 (config 2) and BFVDefault(16384) ----
    for n, B in ((4096, 1024), (16384, 256)):
        g = capi.Context.bfv_default(n)
        g.keygen(1)
        L = g.L
        a, nb = rand_ct(g, rng, B, 2, L)
        b, _ = rand_ct(g, rng, B, 2, L)
        out = g.alloc(nb)
        cb = C.c_size_t(B)
        plain = g.upload(rng.integers(0, g.t, size=n, dtype=np.uint64))
        ops = {
            "bfv%d_mul_relin" % n: lambda: g.op("mul_relin", a.ptr, b.ptr, out.ptr, L, cb),
            "bfv%d_rotate_1" % n: lambda: g.op("rotate", a.ptr, out.ptr, L, 1, cb),
            "bfv%d_add" % n: lambda: g.op("add", a.ptr, b.ptr, out.ptr, 2, L, cb),
            "bfv%d_multiply_plain" % n: lambda: g.op("multiply_plain", a.ptr, plain.ptr, C.c_size_t(0), out.ptr, 2, L, cb),
        }
        # decrypt and the invariant noise budget of the same batch: the budget runs decrypt's transforms, then the exact lift and
        # the maximum in place of the rounding, and reads B ints back (its one synchronisation is inside the timed call)
        dec, budgets = g.alloc(B * n * 8), (C.c_int * B)()
        ops["bfv%d_decrypt" % n] = lambda: g.op("decrypt", a.ptr, 2, L, dec.ptr, cb)
        ops["bfv%d_noise_budget" % n] = lambda: g.op("noise_budget", a.ptr, 2, L, budgets, cb)
        # OS-keyed encryption of the batch (abc_hip_encrypt_secure: getrandom + ChaCha20 sampling on the device, or by the keyed
        # spec's single-threaded host twin under ABC_HIP_HOST_SAMPLING=1) and, on the reference's default ring, a whole key set (abc_hip_keygen_secure: batch 1)
        plains = g.upload(rng.integers(0, g.t, size=(B, n), dtype=np.uint64))
        ops["bfv%d_encrypt_secure" % n] = lambda: g.op("encrypt_secure", plains.ptr, out.ptr, cb)
        # the sampling alone, key upload included: the draws of that batch, and the uniform polynomials of one key-switching key
        key = bytes(range(32))
        ops["bfv%d_keyed_small(draws of encrypt_secure)" % n] = lambda: g.op("keyed_small", key, C.c_uint64(0), out.ptr, cb)
        ops["bfv%d_keyed_uniform(one key: L x K limbs)" % n] = lambda: g.op("keyed_uniform", key, C.c_uint64(2), L, out.ptr)
        for k, fn in ops.items():
            if only not in k:
                continue
            ms = timeit(g, fn)
            res[k] = {"batch": B, "ms": ms, "ops_per_s": B / ms * 1e3}
            print("%-40s %8.3f ms / %d  -> %10.0f op/s" % (k, ms, B, B / ms * 1e3), flush=True)
        if n == 16384 and only in "bfv16384_keygen_secure":
            ms = timeit(g, lambda: g.keygen(None), reps=3)
            res["bfv16384_keygen_secure"] = {"batch": 1, "ms": ms, "ops_per_s": 1e3 / ms}
            print("%-40s %8.3f ms (sk, pk, relin, %d Galois keys)" % ("bfv16384_keygen_secure", ms, len(g.galois_elts())), flush=True)
        if only:
            del a, b, out, dec, plains
            g.close()
            continue
        # single-ciphertext latency (what the C++ plugin shim sees)
        one = C.c_size_t(1)
        ms = timeit(g, lambda: g.op("mul_relin", a.ptr, b.ptr, out.ptr, L, one), reps=20)
        res["bfv%d_mul_relin_latency_ms" % n] = ms
        print("%-40s %8.3f ms (batch 1)" % ("bfv%d_mul_relin latency" % n, ms), flush=True)
        # the same call replayed from a captured HIP graph (abc_hip_graph_*)
        g.op("mul_relin", a.ptr, b.ptr, out.ptr, L, one)  # scratch arenas sized before capture
        g.sync()
        g.graph_begin()
        g.op("mul_relin", a.ptr, b.ptr, out.ptr, L, one)
        ge = g.graph_end()
        ms = timeit(g, lambda: g.graph_launch(ge), reps=20)
        g.graph_destroy(ge)
        res["bfv%d_mul_relin_graph_latency_ms" % n] = ms
        print("%-40s %8.3f ms (batch 1, HIP graph replay)" % ("bfv%d_mul_relin latency" % n, ms), flush=True)
        del a, b, out, dec, plains
        g.close()


def const_sum_ab(res, only, rng):
    """sum over K terms of c_k * ct_k for scalar constants c_k, alternating in one process, five runs each:
    (a) `composed`: K x abc_hip_multiply_plain and K - 1 x abc_hip_add on pre-filled constant plaintexts ([nl][N], every word of a limb equal);
    (b) `plain_sum`: abc_hip_multiply_plain_sum on the same plaintexts;
    (c) `const_sum`: abc_hip_multiply_const_sum, the weights in the kernel arguments;
    and with one rescale behind the sum: (d) `plain_sum_rescale`: abc_hip_multiply_plain_sum_rescale on the plaintexts, as its route sends
    it; then abc_hip_multiply_const_sum_rescale three ways: (e) `csr_separate` under ABC_HIP_CONST_SUM_RESCALE_FUSED=0, (f) `csr_fused`
    under =1 (separate all the same beyond four terms and at N = 2^15), (g) `csr_default`, as route_const_sum_rescale sends it (the rule
    these numbers gave).
    The K ciphertext operands are distinct buffers (device copies of one random batch: the kernels have no data-dependent path)."""
    shapes = [  # tag, context, levels, batches
        ("ckks14", lambda: capi.Context(capi.CKKS, 16384, capi.create_primes(16384, [50, 40, 40, 40, 50])), (4, 3), (512, 128, 64, 32)),
        ("ckks15", lambda: capi.Context(capi.CKKS, 32768, capi.create_primes(32768, [50, 40, 40, 50])), (3,), (256,)),
        ("ckks12", lambda: capi.Context(capi.CKKS, 4096, capi.create_primes(4096, [50, 40, 40, 50])), (3,), (1024, 128)),
    ]
    kinds = ("composed", "plain_sum", "const_sum", "plain_sum_rescale", "csr_separate", "csr_fused", "csr_default")
    u64p = C.POINTER(C.c_uint64)
    for tag, make, levels, batches in shapes:
        if only and only not in "%s_const_sum" % tag and "const_sum" not in only:
            continue
        g = make()
        for nl in levels:
            for B in batches:
                cb, zero = C.c_size_t(B), C.c_size_t(0)
                first, nb = rand_ct(g, rng, B, 2, nl)
                pool = [first]
                for _ in range(15):
                    pool.append(g.alloc(nb))
                    g.op("memcpy_d2d", pool[-1].ptr, first.ptr, C.c_size_t(nb))
                w = np.stack([g.const_words(v, 2.0 ** 40, nl) for v in rng.uniform(-1, 1, 16)])
                plains = [g.upload(np.ascontiguousarray(np.repeat(w[k][:, None], g.n, axis=1))) for k in range(16)]
                tmp, out = g.alloc(nb), g.alloc(nb)
                for K in (1, 2, 4, 8, 16):
                    names = ["%s_L%d_b%d_const_sum_K%d_%s" % (tag, nl, B, K, kind) for kind in kinds]
                    if not any(only in k for k in names):
                        continue
                    pc, pp = g.term_pointers([x.ptr for x in pool[:K]]), g.term_pointers([x.ptr for x in plains[:K]])
                    wk = np.ascontiguousarray(w[:K])
                    wp = wk.ctypes.data_as(u64p)

                    def composed():
                        g.op("multiply_plain", pool[0].ptr, plains[0].ptr, zero, out.ptr, 2, nl, cb)
                        for k in range(1, K):
                            g.op("multiply_plain", pool[k].ptr, plains[k].ptr, zero, tmp.ptr, 2, nl, cb)
                            g.op("add", out.ptr, tmp.ptr, out.ptr, 2, nl, cb)

                    def plain_sum():
                        g.op("multiply_plain_sum", pc, pp, zero, K, None, out.ptr, 2, nl, cb)

                    def const_sum():
                        g.op("multiply_const_sum", pc, None, wp, K, None, None, out.ptr, 2, nl, cb)

                    def plain_sum_rescale():
                        g.op("multiply_plain_sum_rescale", pc, pp, zero, K, None, out.ptr, 2, nl, cb)

                    def const_sum_rescale():
                        g.op("multiply_const_sum_rescale", pc, None, wp, K, None, None, out.ptr, 2, nl, cb)
                    routes = ("composed", "macsum=kernel", "constmac=kernel", g.route("plain_sum_rescale", nl, B) + (" (more than four terms: separate)" if K > 4 else ""))
                    reps = 10 if B * K >= 256 else 50
                    _rounds(g, res, names[:4], (composed, plain_sum, const_sum, plain_sum_rescale), routes, B, reps)
                    key = "ABC_HIP_CONST_SUM_RESCALE_FUSED"
                    _env_rounds(g, res, names[4:], (const_sum_rescale,) * 3, ({key: "0"}, {key: "1"}, {}), "const_sum_rescale", nl, B, reps)
                    med = lambda i: res[names[i]]["ms_median"]  # noqa: E731
                    print("    plain_sum / const_sum: %.2f;  csr_separate / csr_fused: %.2f;  csr_separate / csr_default: %.2f;  plain_sum_rescale / csr_default: %.2f%s" % (
                        med(1) / med(2), med(4) / med(5), med(4) / med(6), med(3) / med(6), "  (K > 4: every csr row is separate)" if K > 4 else ""), flush=True)
                del pool, first, plains, tmp, out
        g.close()


def poly_eval_ab(res, only, rng):
    """c_0 + c_1 x + ... + c_d x^d at N = 2^14 on {50,40,40,40,40,40 | 50}, degree 3 and 7, alternating in one process, five runs each:
    (a) `composed`: the calls a caller writes today on pre-encoded constant plaintexts -- abc_hip_mul_relin, abc_hip_rescale and
        abc_hip_mod_switch per power; abc_hip_multiply_plain, abc_hip_rescale, abc_hip_mod_switch and abc_hip_add per term; abc_hip_add_plain;
    (b) `composed_encode`: the same with the d + 1 abc_hip_ckks_encode calls of the constant vectors in the timed region;
    (c) `poly_eval`: abc_hip_ckks_poly_eval.
    x at 2^40, the result at 2^20 (the constant term enters at out_scale * q_{m-1} < 2^62); the timings do not depend on the values."""
    if only and "poly_eval" not in only:
        return
    n, bits, B = 16384, [50, 40, 40, 40, 40, 40, 50], 128
    g = capi.Context(capi.CKKS, n, capi.create_primes(n, bits))
    g.keygen(5)
    L, N, cb, zero = g.L, g.n, C.c_size_t(B), C.c_size_t(0)
    xs, outs = 2.0 ** 40, 2.0 ** 20
    x, nb = rand_ct(g, rng, B, 2, L)

    def ceil_log2(k):
        e = 0
        while (1 << e) < k:
            e += 1
        return e
    for d in (3, 7):
        names = ["ckks14_L%d_b%d_poly_eval_d%d_%s" % (L, B, d, kind) for kind in ("composed", "composed_encode", "poly_eval")]
        if not any(only in k for k in names):
            continue
        coeffs = [float(v) for v in rng.uniform(-1, 1, d + 1)]
        level, scale, hi, lo = [L] * (d + 1), [xs] * (d + 1), [0] * (d + 1), [0] * (d + 1)
        for k in range(2, d + 1):
            e = ceil_log2(k)
            hi[k], lo[k], level[k] = 1 << (e - 1), k - (1 << (e - 1)), L - e
            scale[k] = scale[hi[k]] * scale[lo[k]] / g.primes[L - e]
        m = L - ceil_log2(d)
        pw = {1: x}
        for k in range(2, d + 1):
            pw[k] = g.alloc(nb)
        sa, sb, acc = g.alloc(nb), g.alloc(nb), g.alloc(nb)
        slots = g.upload(np.stack([np.full(N // 2, c) for c in coeffs]))  # the expanded constant vectors, [d + 1][N / 2] doubles
        plain = [g.alloc(L * N * 8) for _ in range(d + 1)]
        pscale = [outs] + [outs * g.primes[level[k] - 1] / scale[k] for k in range(1, d + 1)]
        plevel = [m - 1] + [level[k] for k in range(1, d + 1)]

        def encode():
            for k in range(d + 1):
                g.op("ckks_encode", C.c_void_p(slots.ptr.value + k * (N // 2) * 8), None, C.c_size_t(N // 2), C.c_double(pscale[k]), plevel[k],
                     plain[k].ptr, C.c_size_t(1))

        def lower(src, frm, to):
            """mod_switch src from `frm` limbs down to `to` through sa / sb; the buffer that holds the result"""
            dst = sa
            while frm > to:
                g.op("mod_switch", src.ptr, dst.ptr, 2, frm, cb)
                src, dst, frm = dst, (sb if dst is sa else sa), frm - 1
            return src

        def composed():
            for k in range(2, d + 1):
                lk = level[k] + 1
                b = lower(pw[lo[k]], level[lo[k]], lk)
                g.op("mul_relin", pw[hi[k]].ptr, b.ptr, acc.ptr, lk, cb)
                g.op("rescale", acc.ptr, pw[k].ptr, 2, lk, cb)
            for k in range(1, d + 1):
                g.op("multiply_plain", pw[k].ptr, plain[k].ptr, zero, sa.ptr, 2, level[k], cb)
                g.op("rescale", sa.ptr, sb.ptr, 2, level[k], cb)
                t = sb
                for frm in range(level[k] - 1, m - 1, -1):
                    u = sa if t is sb else sb
                    g.op("mod_switch", t.ptr, u.ptr, 2, frm, cb)
                    t = u
                if k == 1:
                    g.op("memcpy_d2d", acc.ptr, t.ptr, C.c_size_t(B * 2 * (m - 1) * N * 8))
                else:
                    g.op("add", acc.ptr, t.ptr, acc.ptr, 2, m - 1, cb)
            g.op("add_plain", acc.ptr, plain[0].ptr, zero, acc.ptr, 2, m - 1, cb)

        def composed_encode():
            encode()
            composed()
        co = (C.c_double * (d + 1))(*coeffs)
        out = g.alloc(nb)

        def poly_eval():
            g.op("ckks_poly_eval", x.ptr, C.c_double(xs), co, d, C.c_double(outs), out.ptr, L, cb)
        encode()
        route = g.route("poly_eval", L, B)
        _rounds(g, res, names, (composed, composed_encode, poly_eval), ("composed", "composed", route), B, 5)
    g.close()


def main():
    # --only SUBSTRING: the entries whose name contains it (the contexts of single_ops are still created)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    res = {}
    rng = np.random.default_rng(0)
    # the BFV plaintext-sum A/Bs are named by a prefix of their own, "bfv_plain_sum" / "bfv_matvec_bsgs": a filter that names one of them
    # runs nothing else (and sets up no other context), and a filter that does not say "bfv_" -- `--only matvec_bsgs` -- leaves them out
    bfv_sums = any(x in only for x in ("bfv_plain_sum", "bfv_matvec_bsgs"))
    if not bfv_sums:
        if not (only and any(x in only for x in ("mul_sum", "plain_mac_sum", "matvec_bsgs", "plain_sum_rescale", "const_sum", "poly_eval"))):  # those A/Bs have their own contexts and operand batches: nothing else is set up
            single_ops(res, only, rng)
        rotate_add_ab(res, only, rng)
        rotate_mac_ab(res, only, rng)
        mulplain_rescale_ab(res, only, rng)
        mul_sum_ab(res, only, rng)
        plain_mac_sum_ab(res, only, rng)
        plain_sum_rescale_ab(res, only, rng)
        if "matvec_bsgs_rescale" not in only:  # a filter that names the rescaling form sets up no context of the plain one
            matvec_bsgs_ab(res, only, rng)
        matvec_bsgs_rescale_ab(res, only, rng)
        keyswitch_batch1(res, only, rng)
        const_sum_ab(res, only, rng)
        poly_eval_ab(res, only, rng)
    if not only or "bfv_" in only:
        bfv_plain_sum_ab(res, only, rng)
        bfv_matvec_bsgs_ab(res, only, rng)
    os.makedirs("gpurun_out", exist_ok=True)
    json.dump(res, open("gpurun_out/op_bench.json", "w"), indent=1)


if __name__ == "__main__":
    main()
