#!/usr/bin/env python3
"""Randomised differential check of the C ABI against the CPU oracle (test infrastructure: lives under tests/ because it
uses oracle/; tests/test_gpu_fuzz.py runs short fixed-seed campaigns, the commands below longer ones).  Both sides get the same
random residues (uniform and end-of-range values -- parity is defined on residues, the inputs need not be valid encryptions) and
every output word is compared.  The fixed-parameter tests cover the paths the dispatcher is known to take; this walks the
combinations nobody wrote down (levels 1..L at every ring, odd batches across chunk boundaries, mixed prime sizes, rotations by
arbitrary steps, switches two at a time).

--family base (the default): each round draws a scheme, ring, modulus chain, level, batch size, dispatcher switches and one of
mul_relin, rotate, add, sub, negate, multiply, relinearize, the BFV plaintext operations, CKKS rescale and mod_switch.

--family fused: each round draws a context (scheme, ring 2^10 .. 2^14, chain -- the base family's styles and one with 30-bit
rescaling primes --, a switch set of the base list or of the fused calls' own, two sets at once in one draw of four) and six to ten
operations on it, so that key generation is shared.  The operations are the calls documented as bit-identical to a composition of
base calls, each against that composition on the oracle: rotate_add, apply_galois_add, rotate_sum, rotate_mac_plain, diag_matvec
(o.rotate, o.multiply_plain, o.add); rotate_hoisted, apply_galois_hoisted (hoisted_spec); multiply_sum, mul_sum_relin (mul_sum_spec);
multiply_plain_sum, diag_matvec_bsgs (plain_sum_spec) and their _rescale forms (plain_sum_rescale_spec); bfv_multiply_plain_sum,
bfv_diag_matvec_bsgs (bfv_plain_sum_spec); multiply_const_sum(_rescale) (const_sum_spec); poly_eval (poly_eval_spec);
multiply_plain_rescale and the CKKS multiply_plain, add_plain, sub_plain (the oracle's own calls).  Every level is drawn inside the
call's legal range: a fused case is never skipped.

  python tests/fuzz_parity.py --seconds 60 --seed 1                        (needs a GPU; exits 1 and prints the case on the first mismatch)
  python tests/fuzz_parity.py --family fused --seconds 600 --seed N        (the same for the fused family)
  python tests/fuzz_parity.py --case '{...}' [--also NAME=1,NAME=1]         (replays one printed case, with further switches)
  python tests/fuzz_parity.py --family fused --dry-run --max-cases 200     (no library, no GPU: draws, validates, prints what is covered;
                                                                            --reference evaluates the oracle side up to N = 2^11)
  python tests/fuzz_parity.py --family fused --inject --max-cases 1        (one bit of the result flipped: must end with MISMATCH, exit 1)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the *_spec modules of the fused family

SWITCH_SETS = [
    {}, {}, {}, {},  # the default path gets most of the draws
    {"ABC_HIP_CHUNK": "3", "ABC_HIP_LANES": "2"},
    {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": "1"},
    {"ABC_HIP_NO_FP64": "1"},
    {"ABC_HIP_NO_MIXED": "1"},
    {"ABC_HIP_NO_ISPLIT": "1"},
    {"ABC_HIP_NO_SPLIT": "1"},
    {"ABC_HIP_NO_SPLIT4": "1"},
    {"ABC_HIP_NO_PACK": "1"},
    {"ABC_HIP_NO_KEY_TWIN": "1"},
    {"ABC_HIP_NO_BMUL": "1"},
    {},
    {},
    {"ABC_HIP_NO_IKS": "1"},
    {"ABC_HIP_NO_GALOIS_FUSION": "1"},
    {},
    {"ABC_HIP_NO_LEAN_FRONT": "1"},
    {"ABC_HIP_NO_FUSED": "1"},
    {"ABC_HIP_NO_BSPLIT": "1"},
    {"ABC_HIP_NO_GSPLIT": "1"},
    {"ABC_HIP_NO_TENSOR_INTT": "1"},
    {"ABC_HIP_BEHZ_SEAL_BASE": "1"},
    {"ABC_HIP_BFV_SCRATCH_MB": "64"},
    {"ABC_HIP_FEW_LIMBS": "0"},
]
ALL_SWITCHES = sorted({k for s in SWITCH_SETS for k in s})


def random_ct(rng, primes, nl, n, batch, size=2):
    ct = np.empty((batch, size, nl, n), dtype=np.uint64)
    for j in range(nl):
        q = int(primes[j])
        ct[:, :, j, :] = rng.integers(0, q, size=(batch, size, n), dtype=np.uint64)
        pool = np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1], dtype=np.uint64)
        edge = rng.integers(0, 32, size=(batch, size, n))
        ct[:, :, j, :] = np.where(edge < 6, pool[np.minimum(edge, 5)], ct[:, :, j, :])
    if rng.integers(0, 4) == 0:  # a long run of q - 1: where lazy bounds break first
        ct[0, 0, :, : n // 4] = np.array([int(p) - 1 for p in primes[:nl]], dtype=np.uint64)[:, None]
    return ct


def draw_case(rng, max_logn):
    scheme = "bfv" if rng.integers(0, 2) else "ckks"
    logn = int(rng.choice([12, 12, 13, 13, 14, 14, 14, 15][: 8 if max_logn >= 15 else 7]))
    logn = min(logn, max_logn)
    n = 1 << logn
    case = {"scheme": scheme, "logn": logn, "switches": dict(SWITCH_SETS[int(rng.integers(0, len(SWITCH_SETS)))])}
    if scheme == "bfv":
        if rng.integers(0, 3) and logn <= 14:
            case["bits"] = None  # BFVDefault(n)
        else:
            L = int(rng.integers(1, 5 if logn < 15 else 4))
            b = int(rng.choice([36, 40, 45, 49, 50, 52, 55, 58]))
            case["bits"] = [b] * L + [min(b + 1, 60)]
    else:
        L = int(rng.integers(1, 8)) if rng.integers(0, 3) == 0 else int(rng.integers(1, 5))  # up to seven data limbs
        style = int(rng.integers(0, 4))
        if style == 0:
            bits = [50] + [40] * (L - 1) + [50]
        elif style == 1:
            bits = [60] + [40] * (L - 1) + [60]
        elif style == 2:
            bits = [int(rng.choice([45, 49, 50])) for _ in range(L + 1)]
        else:
            bits = [int(rng.choice([40, 50, 51, 55, 57, 60])) for _ in range(L + 1)]
        case["bits"] = bits
    case["batch"] = int(rng.choice([1, 1, 2, 3, 5, 7, 9]))
    ops = ["mul_relin", "rotate", "add", "sub", "negate", "multiply", "relinearize"]
    if scheme == "bfv":
        ops += ["multiply_plain", "add_plain", "sub_plain"]
    else:
        ops += ["rescale", "mod_switch"]
    case["op"] = str(rng.choice(ops))
    case["step"] = int(rng.integers(-(n // 2) + 1, n // 2)) if rng.integers(0, 2) else int(rng.choice([1, -1, 2, 3, 7, 64, -24, n // 4]))
    if case["step"] == 0:
        case["step"] = 1
    case["alias"] = int(rng.choice([0, 0, 1, 2]))
    case["level_draw"] = float(rng.random())
    case["data_seed"] = int(rng.integers(0, 2 ** 31))
    return case


def run_case(case, om, capi, contexts, inject=False):
    for k in ALL_SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(case["switches"])
    n = 1 << case["logn"]
    bfv = case["scheme"] == "bfv"
    key = (case["scheme"], case["logn"], tuple(case["bits"]) if case["bits"] else None, tuple(sorted(case["switches"].items())))
    if key not in contexts:
        if len(contexts) >= 6:  # keep device and host memory bounded
            for _, (o_, g_) in list(contexts.items())[:3]:
                g_.close()
            for k in list(contexts)[:3]:
                del contexts[k]
        if bfv:
            primes = om.default_bfv_primes(n) if case["bits"] is None else om.create_primes(n, case["bits"])
            t = om.plain_modulus_batching(n, 20)
            o = om.Oracle(om.BFV, n, primes, t)
            g = capi.Context(capi.BFV, n, primes, t)
        else:
            primes = om.create_primes(n, case["bits"])
            o = om.Oracle(om.CKKS, n, primes)
            g = capi.Context(capi.CKKS, n, primes)
        o.keygen(0xABC00001)
        g.keygen(0xABC00001)  # shared sampling spec: identical keys on both sides
        contexts[key] = (o, g)
    o, g = contexts[key]
    g.reload_env()
    L = len(o.primes) - 1
    nl = L if bfv else 1 + int(case["level_draw"] * L)
    nl = min(max(nl, 1), L)
    rng = np.random.default_rng(case["data_seed"])
    B = case["batch"]
    op = case["op"]
    primes = [int(p) for p in o.primes]
    if op == "relinearize":
        x = random_ct(rng, primes, nl, n, B, size=3)
        got, want = g.relinearize(x), np.stack([o.relinearize(r) for r in x])
    elif op in ("mul_relin", "multiply", "add", "sub"):
        x, y = random_ct(rng, primes, nl, n, B), random_ct(rng, primes, nl, n, B)
        alias = case.get("alias", 0) if op != "multiply" else 0
        if alias:  # the C ABI allows the result to overwrite an operand: 1 = first, 2 = second
            import ctypes as C
            bx, by = g.upload(x), g.upload(y)
            dst = bx if alias == 1 else by
            if op == "mul_relin":
                g.op(op, bx.ptr, by.ptr, dst.ptr, nl, C.c_size_t(B))
            else:
                g.op(op, bx.ptr, by.ptr, dst.ptr, 2, nl, C.c_size_t(B))
            got = g.download(dst, x.shape)
            bx.free(); by.free()
        else:
            got = getattr(g, op)(x, y)
        want = np.stack([getattr(o, op)(a, b) for a, b in zip(x, y)])
    elif op == "negate":
        x = random_ct(rng, primes, nl, n, B)
        got, want = g.negate(x), np.stack([o.negate(r) for r in x])
    elif op == "rotate":
        x = random_ct(rng, primes, nl, n, B)
        step = case["step"]
        if not bfv:
            step = step % (n // 2) or 1
        got, want = g.rotate(x, step), np.stack([o.rotate(r, step) for r in x])
    elif op in ("multiply_plain", "add_plain", "sub_plain"):
        x = random_ct(rng, primes, nl, n, B)
        plain = rng.integers(0, o.t, size=n, dtype=np.uint64)
        got = getattr(g, op)(x, plain)
        want = np.stack([getattr(o, op)(r, plain) for r in x])
    elif op in ("rescale", "mod_switch"):
        if nl < 2:
            return "skip"
        x = random_ct(rng, primes, nl, n, B)
        got, want = getattr(g, op)(x), np.stack([getattr(o, op)(r) for r in x])
    else:
        raise ValueError(op)
    return _verdict(got, want, nl, inject)


def _verdict(got, want, nl, inject):
    if inject:  # the checker's own check: one bit of one downloaded word flipped, which the comparison below must report
        got = np.array(got, dtype=np.uint64)
        got.flat[got.size // 2] ^= np.uint64(1 << 17)
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.argwhere(got != want) if got.shape == want.shape else []
        return "MISMATCH nl=%d: %d words differ%s" % (nl, len(bad), (", first at %s" % (tuple(int(v) for v in bad[0]),)) if len(bad) else "")
    return "ok"


# ---------------------------------------------------------------------------------------------------------------------------
# The fused family: the calls that are documented as bit-identical to a composition of base calls, each against that composition
# on the oracle (tests/*_spec.py).  A round draws one context and six to ten operations on it, so that key generation is shared.
# Nothing below draws from the rng of the base family.

FUSED_SWITCH_SETS = [dict(s) for i, s in enumerate(SWITCH_SETS) if s not in SWITCH_SETS[:i]] + [
    {"ABC_HIP_NO_ROTATE_ADD_FUSION": "1"},
    {"ABC_HIP_NO_ROTATE_MAC_FUSION": "1"},
    {"ABC_HIP_NO_MULPLAIN_RESCALE_FUSION": "1"},
    {"ABC_HIP_NO_TENSOR_SUM": "1"},
    {"ABC_HIP_NO_PLAIN_MAC_SUM": "1"},
    {"ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION": "1"},
    {"ABC_HIP_NO_CONST_MAC_SUM": "1"},
    {"ABC_HIP_MAIN_TWO_PER_CU": "1"},
    {"ABC_HIP_PLAIN_SUM_RESCALE_TERMS": "0"},
    {"ABC_HIP_PLAIN_SUM_RESCALE_TERMS": "1"},
    {"ABC_HIP_PLAIN_SUM_RESCALE_TERMS": "2"},
    {"ABC_HIP_PLAIN_SUM_RESCALE_TERMS": "4"},
    {"ABC_HIP_CONST_SUM_RESCALE_FUSED": "0"},
    {"ABC_HIP_CONST_SUM_RESCALE_FUSED": "1"},
    {"ABC_HIP_LEAN_LIMIT": "0"},
    {"ABC_HIP_PASS0_TARGET_LIMIT": "0"},
]
FUSED_SWITCHES = sorted({k for s in FUSED_SWITCH_SETS for k in s})
FUSED_LOGN = [10, 10, 10, 11, 11, 11, 12, 12, 13, 13, 14, 14]  # weighted towards the small rings: the oracle and the keys are cheap there
BFV_DEFAULT_L = {12: 2, 13: 4, 14: 8, 15: 15}  # data limbs of BFVDefault(2^logn); the single-prime defaults below 2^12 hold no keys
FUSED_BATCHES = [1, 2, 3, 5, 7]
CKKS_KINDS = ["rotate_add", "apply_galois_add", "rotate_sum", "rotate_mac_plain", "diag_matvec", "rotate_hoisted", "apply_galois_hoisted",
              "multiply_sum", "mul_sum_relin", "multiply_plain_sum", "diag_matvec_bsgs", "multiply_const_sum", "multiply_plain", "add_plain",
              "sub_plain"]
CKKS_RESCALING_KINDS = ["multiply_plain_rescale", "multiply_plain_sum_rescale", "diag_matvec_bsgs_rescale", "multiply_const_sum_rescale"]  # nl >= 2
BFV_KINDS = ["rotate_add", "apply_galois_add", "rotate_sum", "rotate_hoisted", "apply_galois_hoisted", "multiply_sum", "mul_sum_relin",
             "bfv_multiply_plain_sum", "bfv_multiply_plain_sum", "bfv_diag_matvec_bsgs", "bfv_diag_matvec_bsgs"]
FUSED_KINDS = sorted(set(CKKS_KINDS + CKKS_RESCALING_KINDS + BFV_KINDS + ["poly_eval"]))
POLY_DEGREES = [1, 2, 3, 4, 5, 7]
# (seed, --max-cases) of the campaigns tests/test_gpu_fuzz.py runs; tests/test_fuzz_cases.py shows on the CPU what they cover together
FUSED_CAMPAIGNS = [(17, 80), (32, 80), (139, 80), (151, 80), (188, 80), (213, 80), (221, 80), (238, 80), (284, 80), (298, 80)]
FUSED_INJECT_SEED = 3  # its first round is an N = 2^10 context
POLY_SCALE = 2.0 ** 30  # the 30-bit style: every weight of the last sum, the constant term at out_scale * q_{m-1} included, stays below 2^62


def _ceil_log2(k):
    return max(int(k) - 1, 0).bit_length()


def fused_limbs(ctx):
    return len(ctx["bits"]) - 1 if ctx["bits"] else BFV_DEFAULT_L[ctx["logn"]]


def fused_kinds(ctx):
    """the kinds a context can run: a rescaling call needs two limbs, poly_eval the 30-bit chain and E + 2 limbs"""
    if ctx["scheme"] == "bfv":
        return list(BFV_KINDS)
    kinds = list(CKKS_KINDS)
    if fused_limbs(ctx) >= 2:
        kinds += CKKS_RESCALING_KINDS
        if ctx["style"] == 4:
            kinds += ["poly_eval"] * 4  # one chain style in five can run it: weighted up so that it is drawn at all
    return kinds


def draw_fused_context(rng, max_logn):
    scheme = "bfv" if rng.integers(0, 3) == 0 else "ckks"
    logn = min(int(rng.choice(FUSED_LOGN + ([15] if max_logn >= 15 else []))), max_logn)
    ctx = {"family": "fused", "scheme": scheme, "logn": logn, "style": -1}
    if scheme == "bfv":
        if rng.integers(0, 3) and 12 <= logn <= 14:
            ctx["bits"] = None  # BFVDefault(n)
        else:
            L = int(rng.integers(1, 5 if logn < 15 else 4))
            b = int(rng.choice([36, 40, 45, 49, 50, 52, 55, 58]))
            ctx["bits"] = [b] * L + [min(b + 1, 60)]
    else:
        L = int(rng.integers(1, 8)) if rng.integers(0, 2) == 0 else int(rng.integers(1, 5))  # up to seven data limbs
        style = int(rng.integers(0, 5))
        if style == 0:
            bits = [50] + [40] * (L - 1) + [50]
        elif style == 1:
            bits = [60] + [40] * (L - 1) + [60]
        elif style == 2:
            bits = [int(rng.choice([45, 49, 50])) for _ in range(L + 1)]
        elif style == 3:
            bits = [int(rng.choice([40, 50, 51, 55, 57, 60])) for _ in range(L + 1)]
        else:
            bits = [50] + [30] * (L - 1) + [50]  # 30-bit rescaling primes: poly_eval and large constants are legal
        ctx["bits"], ctx["style"] = bits, style
    switches = dict(FUSED_SWITCH_SETS[int(rng.integers(0, len(FUSED_SWITCH_SETS)))])
    if rng.integers(0, 4) == 0:  # two sets at once: compatibility is not filtered, the library owes the oracle's words under any combination
        switches.update(FUSED_SWITCH_SETS[int(rng.integers(0, len(FUSED_SWITCH_SETS)))])
    ctx["switches"] = switches
    ctx["ops"] = int(rng.integers(6, 11))
    return ctx


def _draw_step(rng, ctx, zero_ok=True, own_key=False):
    """a rotation step: mostly +-2^k (a key of its own), sometimes 0, sometimes a step that runs a NAF chain of keys"""
    n = 1 << ctx["logn"]
    kind = int(rng.integers(0, 8))
    if kind == 0 and zero_ok:
        return 0
    if kind <= 5 or own_key:
        return int(rng.choice([1, -1])) * (1 << int(rng.integers(0, ctx["logn"] - 1)))
    step = int(rng.choice([3, 7, 5, -24, 0])) or int(rng.integers(-(n // 2) + 1, n // 2))
    if ctx["scheme"] == "ckks":
        step %= n // 2  # as the base family asks for CKKS rotations
    return step or 1


def _draw_level(rng, lo, L):
    pick = int(rng.integers(0, 4))
    return lo if pick == 0 else L if pick == 1 else int(rng.integers(lo, L + 1))


def draw_fused_op(rng, ctx):
    """one operation on a drawn context, as a case that carries the context draw with it: --case replays it alone"""
    L, bfv, n = fused_limbs(ctx), ctx["scheme"] == "bfv", 1 << ctx["logn"]
    kinds = fused_kinds(ctx)
    kind = kinds[int(rng.integers(0, len(kinds)))]
    case = {k: v for k, v in ctx.items() if k != "ops"}
    case["switches"] = dict(ctx["switches"])
    case["kind"], case["batch"] = kind, int(rng.choice(FUSED_BATCHES))
    lo = 2 if kind in CKKS_RESCALING_KINDS else 1
    form3 = lambda: str(rng.choice(["bcast", "per", "wide"]))  # noqa: E731
    if kind == "poly_eval":
        case["degree"] = int(rng.choice([d for d in POLY_DEGREES if _ceil_log2(d) + 2 <= L]))
        lo = _ceil_log2(case["degree"]) + 2
    case["nl"] = L if bfv else _draw_level(rng, lo, L)
    if kind == "rotate_add":
        case["step"] = _draw_step(rng, ctx)
    elif kind == "apply_galois_add":
        case["conj"], case["pick"] = int(rng.integers(0, 3) == 0), int(rng.integers(0, 64))
    elif kind == "rotate_sum":
        case["steps"] = [_draw_step(rng, ctx) for _ in range(int(rng.integers(0, 4)))]
    elif kind == "rotate_mac_plain":
        case["step"], case["form"], case["addend"] = _draw_step(rng, ctx), form3(), int(rng.integers(0, 4) != 0)
    elif kind == "diag_matvec":
        case["steps"], case["wide"] = [_draw_step(rng, ctx) for _ in range(int(rng.integers(0, 5)))], int(rng.integers(0, 2))
    elif kind == "rotate_hoisted":
        case["steps"] = [_draw_step(rng, ctx, own_key=True) for _ in range(int(rng.integers(1, 6)))]
    elif kind == "apply_galois_hoisted":
        case["picks"] = [int(rng.integers(0, 64)) for _ in range(int(rng.integers(1, 6)))]  # indices into galois_elts(); duplicates allowed
    elif kind in ("multiply_sum", "mul_sum_relin"):
        K = int(rng.choice([1, 2, 3, 5, 8, 9]))
        case["pool"] = int(rng.integers(1, min(K, 3) + 2))  # distinct ciphertexts; a term picks two of them, so squares and repeats occur
        case["terms"] = [[int(rng.integers(0, case["pool"])), int(rng.integers(0, case["pool"]))] for _ in range(K)]
        if bfv and ctx["logn"] >= 13:  # the oracle's BEHZ product takes 0.2 s at N = 2^14: hold K * batch where a case stays a few seconds
            while K * case["batch"] > 10 and case["batch"] > 1:
                case["batch"] = FUSED_BATCHES[FUSED_BATCHES.index(case["batch"]) - 1]
    elif kind in ("multiply_plain_sum", "multiply_plain_sum_rescale"):
        K = int(rng.choice([1, 2, 3, 4, 5, 8, 9]))
        case["pool"] = int(rng.integers(1, min(K, 3) + 1))
        case["terms"] = [[int(rng.integers(0, case["pool"])), int(rng.integers(0, case["pool"]))] for _ in range(K)]  # (ciphertext, plaintext)
        case["form"], case["addend"], case["size"] = form3(), int(rng.integers(0, 2)), int(rng.choice([2, 2, 3]))
    elif kind in ("diag_matvec_bsgs", "diag_matvec_bsgs_rescale", "bfv_diag_matvec_bsgs"):
        case["baby"] = [_draw_step(rng, ctx) for _ in range(int(rng.integers(1, 4)))]
        case["giant"] = [_draw_step(rng, ctx) for _ in range(int(rng.integers(1, 4)))]
        case["wide"] = int(rng.integers(0, 2))
    elif kind == "bfv_multiply_plain_sum":
        K = int(rng.choice([1, 2, 3, 5, 8, 9]))
        case["pool"] = int(rng.integers(1, min(K, 3) + 1))
        case["terms"] = [[int(rng.integers(0, case["pool"])), int(rng.integers(0, case["pool"]))] for _ in range(K)]
        case["ct_form"], case["per"], case["addend"], case["size"] = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.choice([2, 2, 3]))
        case["plain"] = "lifted" if case["ct_form"] == 0 and rng.integers(0, 2) else "residues"
        if case["plain"] == "residues":  # the reference is Python-integer arithmetic per word: hold a case near a second
            while case["batch"] * case["size"] * L * K * n > 4e6 and case["batch"] > 1:
                case["batch"] = FUSED_BATCHES[FUSED_BATCHES.index(case["batch"]) - 1]
    elif kind in ("multiply_const_sum", "multiply_const_sum_rescale"):
        K = int(rng.choice([0, 1, 2, 3, 4, 5, 8, 9]))
        case["pool"] = int(rng.integers(1, 4))
        case["terms"] = [int(rng.integers(0, case["pool"])) for _ in range(K)]
        case["pool_nl"] = [_draw_level(rng, case["nl"], L) for _ in range(case["pool"])]  # every term is read at its own level
        case["const"], case["addend"], case["size"] = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.choice([2, 2, 3]))
        # d_out may BE d_addend where the shapes agree: not behind a rescale
        case["out_is_addend"] = int(kind == "multiply_const_sum" and case["addend"] and rng.integers(0, 2) == 0)
    elif kind in ("multiply_plain_rescale", "multiply_plain", "add_plain", "sub_plain"):
        case["form"], case["size"] = form3() if kind == "multiply_plain_rescale" else str(rng.choice(["bcast", "per"])), int(rng.choice([2, 2, 3]))
    case["data_seed"] = int(rng.integers(0, 2 ** 31))
    return case


def draw_fused_round(rng, max_logn):
    ctx = draw_fused_context(rng, max_logn)
    return [draw_fused_op(rng, ctx) for _ in range(ctx["ops"])]


def validate_fused(case):
    """what a drawn case must satisfy before any library sees it; raises on the first violation"""
    L = fused_limbs(case)
    kind, nl = case["kind"], case["nl"]
    assert kind in fused_kinds(case), "%s cannot run on this context" % kind
    assert case["batch"] in FUSED_BATCHES and 10 <= case["logn"] <= 15
    assert 1 <= nl <= L and (case["scheme"] == "ckks" or nl == L), "level %d outside 1..%d" % (nl, L)
    assert kind not in CKKS_RESCALING_KINDS or nl >= 2, "a rescaling call below two limbs"
    if kind == "poly_eval":
        assert case["style"] == 4 and nl >= _ceil_log2(case["degree"]) + 2, "poly_eval below E + 2 limbs"
    for key in FUSED_SWITCHES:
        assert case["switches"].get(key, "0").isdigit()
    assert all(nl <= v <= L for v in case.get("pool_nl", [])), "a term below the sum's level"
    half = 1 << (case["logn"] - 1)
    steps = list(case.get("steps", [])) + list(case.get("baby", [])) + list(case.get("giant", [])) + [case.get("step", 0)]
    assert all(abs(s) < half for s in steps), "a step past N / 2"
    if kind == "rotate_hoisted":
        assert all(s == 0 or abs(s) & (abs(s) - 1) == 0 for s in steps), "a hoisted step needs a key of its own"


def _plains(rng, primes, rows, n, count):
    """[count][rows][N] plaintext residues: random_ct's treatment per limb"""
    return random_ct(rng, primes, rows, n, count, size=1)[:, 0]


def _poly_coeffs(rng, primes, nl, degree):
    """coefficients redrawn, in the order of the data rng, until the plan's every weight is legal (const_words raises past 2^62)"""
    import poly_eval_spec
    for _ in range(64):
        coeffs = [float(v) for v in rng.uniform(-1.0, 1.0, size=degree + 1)]
        for k in range(degree):  # a zero coefficient leaves a term, and perhaps a power, out: never the leading one
            if rng.integers(0, 6) == 0:
                coeffs[k] = 0.0
        try:
            poly_eval_spec.plan(primes, nl, POLY_SCALE, coeffs, POLY_SCALE)
            return coeffs
        except ValueError:
            continue
    raise ValueError("no legal coefficients in 64 draws")


def fused_io(case, o):
    """inputs of a fused case, drawn from data_seed, and both sides of it: (dev, ref, out_shape).  dev(g) is the device call on a
    capi.Context, ref() its restatement on the oracle; out_shape is what the header promises."""
    import bfv_plain_sum_spec
    import const_sum_spec
    import hoisted_spec
    import mul_sum_spec
    import plain_sum_rescale_spec
    import plain_sum_spec
    import poly_eval_spec
    kind, nl, B, n = case["kind"], case["nl"], case["batch"], 1 << case["logn"]
    L = o.L
    assert L == fused_limbs(case)
    primes = [int(p) for p in o.primes]
    rng = np.random.default_rng(case["data_seed"])
    ct = lambda level=nl, size=2: random_ct(rng, primes, level, n, B, size)  # noqa: E731
    rows = lambda f: np.stack([f(i) for i in range(B)])  # noqa: E731

    def plain_operand(form):
        """(what the device wrapper takes, row i of it as the oracle takes it)"""
        if form == "bcast":
            p = _plains(rng, primes, nl, n, 1)[0]
            return p, lambda i: p
        p = _plains(rng, primes, L if form == "wide" else nl, n, B)
        return p, lambda i: np.ascontiguousarray(p[i, :nl])

    def elts():
        have = o.galois_elts()
        assert have, "the context holds no Galois key"
        return have

    def rot(c, s):
        return o.rotate(c, s) if s else c

    if kind == "rotate_add":
        x, a, s = ct(), ct(), case["step"]
        return (lambda g: g.rotate_add(x, a, s)), (lambda: rows(lambda i: o.add(a[i], rot(x[i], s)))), x.shape
    if kind == "apply_galois_add":
        x, a = ct(), ct()
        e = 2 * n - 1 if case["conj"] else elts()[case["pick"] % len(elts())]
        return (lambda g: g.apply_galois_add(x, a, e)), (lambda: rows(lambda i: o.add(a[i], o.apply_galois(x[i], e)))), x.shape
    if kind == "rotate_sum":
        x, steps = ct(), case["steps"]

        def tree(c):
            for s in steps:
                c = o.add(c, rot(c, s))
            return c
        return (lambda g: g.rotate_sum(x, steps)), (lambda: rows(lambda i: tree(x[i]))), x.shape
    if kind == "rotate_mac_plain":
        x, a, s = ct(), (ct() if case["addend"] else None), case["step"]
        p, prow = plain_operand(case["form"])

        def mac(i):
            prod = o.multiply_plain(rot(x[i], s), prow(i))
            return prod if a is None else o.add(a[i], prod)
        return (lambda g: g.rotate_mac_plain(x, p, a, s)), (lambda: rows(mac)), x.shape
    if kind == "diag_matvec":
        x, steps = ct(), case["steps"]
        d = _plains(rng, primes, L if case["wide"] else nl, n, max(len(steps), 1))[: len(steps)]
        return (lambda g: g.diag_matvec(x, d, steps)), (lambda: rows(lambda i: plain_sum_spec.diag_matvec(o, x[i], d, steps))), x.shape
    if kind in ("rotate_hoisted", "apply_galois_hoisted"):
        x = ct()
        if kind == "rotate_hoisted":
            items = case["steps"]
            es = [o.elt_from_step(s) if s else 0 for s in items]
        else:
            items = es = [elts()[p % len(elts())] for p in case["picks"]]
        keys = {e: hoisted_spec.permuted_key(o, e) for e in set(es) if e}

        def ref():
            return np.stack([rows(lambda i: hoisted_spec.hoisted_reference(o, x[i], e, keys[e]) if e else x[i]) for e in es])
        return (lambda g: getattr(g, kind)(x, items)), ref, (len(items),) + x.shape
    if kind in ("multiply_sum", "mul_sum_relin"):
        pool = [ct() for _ in range(case["pool"])]
        as_, bs = [pool[a] for a, _ in case["terms"]], [pool[b] for _, b in case["terms"]]
        f = getattr(mul_sum_spec, kind)
        return (lambda g: getattr(g, kind)(as_, bs)), (lambda: rows(lambda i: f(o, [a[i] for a in as_], [b[i] for b in bs], nl))), \
            (B, 3 if kind == "multiply_sum" else 2, nl, n)
    if kind in ("multiply_plain_sum", "multiply_plain_sum_rescale"):
        size, drop = case["size"], int(kind.endswith("rescale"))
        cpool = [ct(size=size) for _ in range(case["pool"])]
        ppool = [plain_operand(case["form"]) for _ in range(case["pool"])]
        a = ct(size=size) if case["addend"] else None
        cts, pls = [cpool[c] for c, _ in case["terms"]], [ppool[p] for _, p in case["terms"]]
        f = getattr(plain_sum_rescale_spec if drop else plain_sum_spec, kind)
        return (lambda g: getattr(g, kind)(cts, [p[0] for p in pls], addend=a)), \
            (lambda: rows(lambda i: f(o, [c[i] for c in cts], [p[1](i) for p in pls], addend=None if a is None else a[i], size=size, nl=nl))), \
            (B, size, nl - drop, n)
    if kind in ("diag_matvec_bsgs", "diag_matvec_bsgs_rescale"):
        x, baby, giant, drop = ct(), case["baby"], case["giant"], int(kind.endswith("rescale"))
        d = _plains(rng, primes, L if case["wide"] else nl, n, len(baby) * len(giant))
        f = getattr(plain_sum_rescale_spec if drop else plain_sum_spec, kind)
        return (lambda g: getattr(g, kind)(x, d, baby, giant)), (lambda: rows(lambda i: f(o, x[i], d, baby, giant))), (B, 2, nl - drop, n)
    if kind == "bfv_diag_matvec_bsgs":
        x, baby, giant = ct(), case["baby"], case["giant"]
        d = random_ct(rng, [o.t], 1, n, len(baby) * len(giant), size=1)[:, 0, 0]  # [rows][N] mod t
        return (lambda g: g.bfv_diag_matvec_bsgs(x, g.bfv_plain_to_ntt(d), baby, giant)), \
            (lambda: rows(lambda i: bfv_plain_sum_spec.diag_matvec_bsgs(o, x[i], list(d), baby, giant))), x.shape
    if kind == "bfv_multiply_plain_sum":
        size, per = case["size"], case["per"]
        cpool = [ct(size=size) for _ in range(case["pool"])]
        if case["plain"] == "lifted":  # plaintexts modulo t, transformed by the spec: the reference is the oracle's own multiply_plain and add
            praw = [random_ct(rng, [o.t], 1, n, B if per else 1, size=1)[:, 0, 0] for _ in range(case["pool"])]
            ppool = [np.stack([bfv_plain_sum_spec.plain_to_ntt(o, r) for r in p]) for p in praw]
        else:
            ppool = [_plains(rng, primes, L, n, B if per else 1) for _ in range(case["pool"])]
        a = ct(size=size) if case["addend"] else None
        cts = [cpool[c] for c, _ in case["terms"]]
        pls = [ppool[p] if per else ppool[p][0] for _, p in case["terms"]]

        def ref(i):
            ai = None if a is None else a[i]
            if case["plain"] == "lifted":
                return bfv_plain_sum_spec.composed_sum(o, [c[i] for c in cts], [praw[p][i if per else 0] for _, p in case["terms"]], ai)
            return bfv_plain_sum_spec.multiply_plain_sum(o, [c[i] for c in cts], [p[i] if per else p for p in pls], ai, case["ct_form"], size)
        return (lambda g: g.bfv_multiply_plain_sum(cts, pls, addend=a, ct_form=case["ct_form"])), (lambda: rows(ref)), (B, size, L, n)
    if kind in ("multiply_const_sum", "multiply_const_sum_rescale"):
        size, drop, K = case["size"], int(kind.endswith("rescale")), len(case["terms"])
        pool = [ct(level=lv, size=size) for lv in case["pool_nl"]]
        cts = [pool[t] for t in case["terms"]]
        words = _plains(rng, primes, nl, 1, K + 1)[:, :, 0]  # [K + 1][nl] words below their primes, the ends of the range among them
        weights, const = words[:K], (words[K] if case["const"] else None)
        a = ct(size=size) if case["addend"] else None
        f = getattr(const_sum_spec, kind)

        def dev(g):
            if not case["out_is_addend"]:
                return getattr(g, kind)(cts, weights, const=const, addend=a, size=size, nl=nl, count=B)
            import ctypes as C
            bufs = {}
            for c in cts:
                if id(c) not in bufs:
                    bufs[id(c)] = g.upload(c)
            ab = g.upload(a)
            try:
                l, w, k = g.const_sum_args(weights, const, [c.shape[2] for c in cts], K, nl)
                g.op(kind, g.term_pointers([bufs[id(c)].ptr for c in cts]), l, w.ctypes.data_as(C.POINTER(C.c_uint64)), K,
                     None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64)), ab.ptr, ab.ptr, size, nl, C.c_size_t(B))
                return g.download(ab, a.shape)
            finally:
                for b in list(bufs.values()) + [ab]:
                    b.free()
        return dev, (lambda: rows(lambda i: f(o, [c[i] for c in cts], weights, const=const, addend=None if a is None else a[i], size=size, nl=nl))), \
            (B, size, nl - drop, n)
    if kind == "poly_eval":
        coeffs = _poly_coeffs(rng, primes, nl, case["degree"])
        x = ct()
        return (lambda g: g.poly_eval(x, POLY_SCALE, coeffs, POLY_SCALE)), \
            (lambda: rows(lambda i: poly_eval_spec.poly_eval(o, x[i], POLY_SCALE, coeffs, POLY_SCALE))), (B, 2, nl - poly_eval_spec.depth(case["degree"]), n)
    if kind == "multiply_plain_rescale":
        x = ct(size=case["size"])
        p, prow = plain_operand(case["form"])
        return (lambda g: g.multiply_plain_rescale(x, p)), (lambda: rows(lambda i: o.rescale(o.multiply_plain(x[i], prow(i))))), \
            (B, case["size"], nl - 1, n)
    if kind in ("multiply_plain", "add_plain", "sub_plain"):
        x = ct(size=case["size"])
        p, prow = plain_operand(case["form"])
        return (lambda g: getattr(g, kind)(x, p)), (lambda: rows(lambda i: getattr(o, kind)(x[i], prow(i)))), x.shape
    raise ValueError(kind)


def fused_oracle(case, om):
    n = 1 << case["logn"]
    if case["scheme"] == "bfv":
        primes = om.default_bfv_primes(n) if case["bits"] is None else om.create_primes(n, case["bits"])
        o = om.Oracle(om.BFV, n, primes, om.plain_modulus_batching(n, 20))
    else:
        o = om.Oracle(om.CKKS, n, om.create_primes(n, case["bits"]))
    o.keygen(0xABC00001)
    return o


def fused_context_key(case):
    return (case["scheme"], case["logn"], tuple(case["bits"]) if case["bits"] else None, tuple(sorted(case["switches"].items())))


def run_fused_case(case, om, capi, contexts, inject=False):
    """capi None: the oracle side alone (--dry-run --reference): it must run, give the header's shape and words below their primes"""
    validate_fused(case)
    for k in set(ALL_SWITCHES) | set(FUSED_SWITCHES):
        os.environ.pop(k, None)
    os.environ.update(case["switches"])
    key = fused_context_key(case)
    if key not in contexts:
        for _, g_ in contexts.values():  # one round, one context: the one before is done
            if g_ is not None:
                g_.close()
        contexts.clear()
        o = fused_oracle(case, om)
        g = None
        if capi is not None:
            g = capi.Context(capi.BFV if case["scheme"] == "bfv" else capi.CKKS, o.n, o.primes, o.t)
            g.keygen(0xABC00001)  # shared sampling spec: identical keys on both sides
        contexts[key] = (o, g)
    o, g = contexts[key]
    dev, ref, shape = fused_io(case, o)
    want = ref()
    assert want.shape == tuple(shape), "the reference's shape %s is not the header's %s" % (want.shape, tuple(shape))
    if g is None:
        for j in range(want.shape[-2]):
            assert int(want[..., j, :].max(initial=0)) < int(o.primes[j]), "a reference word at or above its prime"
        return "ok"
    g.reload_env()
    return _verdict(dev(g), want, case["nl"], inject)


def fused_cases(seed, max_logn, max_cases=0):
    """the cases of a campaign, round after round; max_cases cuts the last round short"""
    rng = np.random.default_rng(seed)
    done = 0
    while not max_cases or done < max_cases:
        for case in draw_fused_round(rng, max_logn):
            if max_cases and done >= max_cases:
                break
            done += 1
            yield case


def prefill_outputs(capi):
    """The GPU side of every case allocates its outputs through Context.alloc (inputs go through upload): from here on each such
    buffer starts as tests/footprint.py's sentinel -- no residue of any prime, different in every word -- instead of whatever the
    block held, so an output word the call leaves unwritten cannot equal the oracle's by being the previous case's.  Host side only:
    no draw and no recorded case changes."""
    import ctypes as C
    import footprint
    plain_alloc = capi.Context.alloc

    def alloc(self, nbytes):
        buf = plain_alloc(self, nbytes)
        fill = footprint.sentinel_words(0, (buf.nbytes + 7) // 8)
        capi._chk(capi.lib().abc_hip_memcpy_h2d(self.h, buf.ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes)))
        return buf
    capi.Context.alloc = alloc


def dry_run(a, om):
    """draw and validate, no library and no GPU: the summary a test reads to see what a campaign covers"""
    out = {"family": a.family, "cases": 0, "skipped": 0, "contexts": 0, "referenced": 0}
    for name in ("by_kind", "by_ring", "by_level", "by_batch", "by_switch", "contexts_by_ring"):
        out[name] = {}
    out.update({"kinds_by_switch": {}, "level_is_top": 0, "level_is_one": 0, "level_max": 0, "batch_over_chunk_lanes": 0, "drawn": []})

    def count(name, key):
        out[name][str(key)] = out[name].get(str(key), 0) + 1
    if a.family == "base":
        rng = np.random.default_rng(a.seed)
        cases = (draw_case(rng, a.max_logn) for _ in range(a.max_cases))
    else:
        cases = fused_cases(a.seed, a.max_logn, a.max_cases)
    last, contexts = None, {}
    for case in cases:
        out["cases"] += 1
        if a.list:
            out["drawn"].append(case)
        if a.family == "base":
            count("by_kind", case["op"]); count("by_ring", case["logn"]); count("by_batch", case["batch"])
            continue
        validate_fused(case)
        if fused_context_key(case) != last:
            last = fused_context_key(case)
            out["contexts"] += 1
            count("contexts_by_ring", case["logn"])
        count("by_kind", case["kind"]); count("by_ring", case["logn"]); count("by_level", case["nl"]); count("by_batch", case["batch"])
        sw = case["switches"]
        for k, v in sw.items():
            count("by_switch", "%s=%s" % (k, v))
            out["kinds_by_switch"]["%s=%s" % (k, v)] = sorted(set(out["kinds_by_switch"].get("%s=%s" % (k, v), [])) | {case["kind"]})
        out["level_is_top"] += case["nl"] == fused_limbs(case) and case["scheme"] == "ckks"
        out["level_is_one"] += case["nl"] == 1
        out["level_max"] = max(out["level_max"], case["nl"] if case["scheme"] == "ckks" else 0)  # BFV has one level: its L says nothing here
        if "ABC_HIP_CHUNK" in sw:
            out["batch_over_chunk_lanes"] += case["batch"] > int(sw["ABC_HIP_CHUNK"]) * int(sw.get("ABC_HIP_LANES", "1"))
        if a.reference and case["logn"] <= 11:
            res = run_fused_case(case, om, None, contexts)
            out["referenced"] += res == "ok"
            out["skipped"] += res == "skip"
    if not a.list:
        del out["drawn"]
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--family", choices=["base", "fused"], default="base", help="fused: the calls documented as compositions of base calls")
    ap.add_argument("--max-logn", type=int, default=14, help="15 adds N = 2^15 (the oracle then needs seconds per draw)")
    ap.add_argument("--max-cases", type=int, default=0)
    ap.add_argument("--case", default="", help="replay one case: the JSON object a failed campaign printed under \"case\"")
    ap.add_argument("--also", default="", help="with --case: extra switches for the replay, NAME=1,NAME=1")
    ap.add_argument("--dry-run", action="store_true", help="draw and validate --max-cases cases and print what they cover: no library, no GPU")
    ap.add_argument("--reference", action="store_true", help="with --dry-run: also evaluate the oracle side of the cases up to N = 2^11")
    ap.add_argument("--list", action="store_true", help="with --dry-run: the drawn cases themselves, under \"drawn\"")
    ap.add_argument("--inject", action="store_true", help="flip one bit of every downloaded result: the campaign must then end with MISMATCH")
    a = ap.parse_args(argv)
    if a.dry_run:
        if not a.max_cases:
            ap.error("--dry-run needs --max-cases")
        om = None
        if a.reference:
            import oracle_py as om
        return dry_run(a, om)
    import oracle_py as om
    from abc_amd import capi
    prefill_outputs(capi)
    if a.case:
        case = json.loads(a.case)
        for kv in filter(None, a.also.split(",")):
            case["switches"][kv.split("=")[0]] = kv.split("=")[1]
        run = run_fused_case if case.get("family") == "fused" else run_case
        print(json.dumps({"result": run(case, om, capi, {}, inject=a.inject), "case": case}), flush=True)
        return
    t0 = last_note = time.time()
    if a.family == "fused":
        cases, run = fused_cases(a.seed, a.max_logn, a.max_cases), run_fused_case
    else:
        rng = np.random.default_rng(a.seed)
        cases, run = iter(lambda: draw_case(rng, a.max_logn), None), run_case
    contexts, counts = {}, {}
    done = skipped = 0
    while time.time() - t0 < a.seconds and (not a.max_cases or done < a.max_cases):
        case = next(cases, None)
        if case is None:
            break
        res = run(case, om, capi, contexts, inject=a.inject)
        done += 1
        skipped += res == "skip"
        tag = "%s/%s" % (case["scheme"], case["op" if a.family == "base" else "kind"])
        counts[tag] = counts.get(tag, 0) + (res == "ok")
        if time.time() - last_note > 60:
            last_note = time.time()
            print("... %d cases, %.0f s" % (done, time.time() - t0), flush=True)
        if res.startswith("MISMATCH"):
            print(json.dumps({"result": res, "case": case}), flush=True)
            sys.exit(1)
    print(json.dumps({"family": a.family, "cases": done, "skipped": skipped, "seconds": round(time.time() - t0, 1), "passed_by_kind": counts}), flush=True)


if __name__ == "__main__":
    main()
