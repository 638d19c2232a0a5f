"""ctypes binding of libabc_hip.so (the C ABI declared in include/abc_hip.h).

Plumbing for tests, bench.py and __graft_entry__: every call goes through the C ABI into the HIP
kernels.  There is NO CPU fallback: a missing library, a missing GPU or a failing call raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ABC_HIP_LIB") or os.path.join(_HERE, "libabc_hip.so")  # override: A/B of two builds

BFV, CKKS = 1, 2
u64p = C.POINTER(C.c_uint64)
i64p = C.POINTER(C.c_int64)

_lib = None

# every symbol include/abc_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "abc_hip_last_error", "abc_hip_device_count", "abc_hip_ctx_create", "abc_hip_ctx_destroy",
    "abc_hip_default_bfv_primes", "abc_hip_plain_modulus_batching", "abc_hip_create_primes", "abc_hip_ctx_info",
    "abc_hip_set_stream", "abc_hip_sync", "abc_hip_ctx_reload_env", "abc_hip_route", "abc_hip_malloc", "abc_hip_free", "abc_hip_trim",
    "abc_hip_cached_bytes", "abc_hip_memcpy_h2d", "abc_hip_memcpy_d2h",
    "abc_hip_memcpy_d2d", "abc_hip_keygen", "abc_hip_keygen_secure", "abc_hip_encrypt_secure", "abc_hip_load_secret_key", "abc_hip_load_public_key",
    "abc_hip_load_relin_key", "abc_hip_load_galois_key", "abc_hip_get_secret_key", "abc_hip_get_public_key",
    "abc_hip_get_relin_key", "abc_hip_get_galois_key", "abc_hip_num_galois_keys", "abc_hip_galois_elt_at",
    "abc_hip_galois_elt_from_step", "abc_hip_batch_encode", "abc_hip_batch_decode", "abc_hip_ckks_encode", "abc_hip_ckks_decode",
    "abc_hip_encrypt", "abc_hip_decrypt", "abc_hip_noise_budget",
    "abc_hip_add", "abc_hip_sub", "abc_hip_negate", "abc_hip_multiply", "abc_hip_relinearize", "abc_hip_mul_relin",
    "abc_hip_rotate", "abc_hip_apply_galois", "abc_hip_multiply_plain", "abc_hip_add_plain", "abc_hip_sub_plain",
    "abc_hip_rescale", "abc_hip_mod_switch", "abc_hip_ntt_forward", "abc_hip_ntt_inverse", "abc_hip_keyswitch",
    "abc_hip_microbench", "abc_hip_timer_start", "abc_hip_timer_stop",
    "abc_hip_ntt_limbs",
    "abc_hip_graph_begin", "abc_hip_graph_end", "abc_hip_graph_launch", "abc_hip_graph_destroy",
    "abc_hip_encrypt_keyed", "abc_hip_keygen_keyed", "abc_hip_keyed_small", "abc_hip_keyed_uniform", "abc_hip_keyed_small_host",
    "abc_hip_apply_galois_hoisted", "abc_hip_rotate_hoisted",
    "abc_hip_rotate_add", "abc_hip_apply_galois_add", "abc_hip_rotate_sum",
    "abc_hip_rotate_mac_plain", "abc_hip_apply_galois_mac_plain", "abc_hip_diag_matvec",
    "abc_hip_multiply_plain_rescale",
    "abc_hip_multiply_sum", "abc_hip_mul_sum_relin",
    "abc_hip_multiply_plain_sum", "abc_hip_rotate_plain", "abc_hip_diag_matvec_bsgs",
    "abc_hip_bfv_plain_to_ntt", "abc_hip_bfv_multiply_plain_sum", "abc_hip_bfv_diag_matvec_bsgs",
    "abc_hip_multiply_plain_sum_rescale", "abc_hip_diag_matvec_bsgs_rescale",
    "abc_hip_ckks_const_words", "abc_hip_multiply_const_sum", "abc_hip_multiply_const_sum_rescale",
    "abc_hip_ckks_poly_eval_depth", "abc_hip_ckks_poly_eval",
]


class AbcHipError(RuntimeError):
    pass


def lib():
    """Load libabc_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AbcHipError("libabc_hip.so is not built: run `python -m abc_amd.build` (hipcc, gfx950)")
        L = C.CDLL(LIB_PATH)
        L.abc_hip_last_error.restype = C.c_char_p
        L.abc_hip_plain_modulus_batching.restype = C.c_uint64
        L.abc_hip_plain_modulus_batching.argtypes = [C.c_size_t, C.c_int]
        L.abc_hip_default_bfv_primes.argtypes = [C.c_size_t, u64p]
        L.abc_hip_create_primes.argtypes = [C.c_size_t, C.POINTER(C.c_int), C.c_int, u64p]
        L.abc_hip_ctx_create.argtypes = [C.c_int, C.c_int, u64p, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
        L.abc_hip_ctx_destroy.argtypes = [C.c_void_p]
        L.abc_hip_galois_elt_at.restype = C.c_uint32
        L.abc_hip_cached_bytes.restype = C.c_size_t
        L.abc_hip_cached_bytes.argtypes = [C.c_void_p]
        L.abc_hip_galois_elt_from_step.restype = C.c_uint32
        L.abc_hip_route.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
        L.abc_hip_apply_galois_hoisted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_size_t]
        L.abc_hip_rotate_hoisted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_size_t]
        L.abc_hip_rotate_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t]
        L.abc_hip_apply_galois_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_size_t]
        L.abc_hip_rotate_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_size_t]
        if hasattr(L, "abc_hip_rotate_mac_plain"):  # not in a build older than these calls (ABC_HIP_LIB: A/B against a parent build)
            L.abc_hip_rotate_mac_plain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t]
            L.abc_hip_apply_galois_mac_plain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_size_t]
            L.abc_hip_diag_matvec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int, C.c_size_t]
        if hasattr(L, "abc_hip_mul_sum_relin"):
            for f in (L.abc_hip_multiply_sum, L.abc_hip_mul_sum_relin):
                f.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_size_t]
        if hasattr(L, "abc_hip_multiply_plain_sum"):
            L.abc_hip_multiply_plain_sum.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_int, C.c_int, C.c_size_t]
            L.abc_hip_rotate_plain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t]
            L.abc_hip_diag_matvec_bsgs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                                   C.c_int, C.c_void_p, C.c_int, C.c_size_t]
        if hasattr(L, "abc_hip_bfv_multiply_plain_sum"):
            L.abc_hip_bfv_plain_to_ntt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
            L.abc_hip_bfv_multiply_plain_sum.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]
            L.abc_hip_bfv_diag_matvec_bsgs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_int,
                                                       C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_size_t]
        if hasattr(L, "abc_hip_multiply_plain_sum_rescale"):
            L.abc_hip_multiply_plain_sum_rescale.argtypes = L.abc_hip_multiply_plain_sum.argtypes
            L.abc_hip_diag_matvec_bsgs_rescale.argtypes = L.abc_hip_diag_matvec_bsgs.argtypes
        if hasattr(L, "abc_hip_multiply_const_sum"):
            L.abc_hip_ckks_const_words.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, u64p]
            L.abc_hip_multiply_const_sum.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), u64p, C.c_int, u64p, C.c_void_p,
                                                     C.c_void_p, C.c_int, C.c_int, C.c_size_t]
            L.abc_hip_multiply_const_sum_rescale.argtypes = L.abc_hip_multiply_const_sum.argtypes
            L.abc_hip_ckks_poly_eval_depth.argtypes = [C.c_int]
            L.abc_hip_ckks_poly_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_void_p,
                                                 C.c_int, C.c_size_t]
        L.abc_hip_encrypt_keyed.argtypes =[C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_size_t]
        L.abc_hip_keygen_keyed.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.abc_hip_keyed_small.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_size_t]
        L.abc_hip_keyed_uniform.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p]
        L.abc_hip_keyed_small_host.argtypes = [C.c_char_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise AbcHipError(lib().abc_hip_last_error().decode())


def default_bfv_primes(n):
    out = (C.c_uint64 * 16)()
    cnt = lib().abc_hip_default_bfv_primes(n, out)
    if cnt < 0:
        raise AbcHipError(lib().abc_hip_last_error().decode())
    return [int(out[i]) for i in range(cnt)]


def plain_modulus_batching(n, bits=20):
    v = int(lib().abc_hip_plain_modulus_batching(n, bits))
    if not v:
        raise AbcHipError(lib().abc_hip_last_error().decode())
    return v


def create_primes(n, bit_sizes):
    out = (C.c_uint64 * len(bit_sizes))()
    bs = (C.c_int * len(bit_sizes))(*bit_sizes)
    _chk(lib().abc_hip_create_primes(n, bs, len(bit_sizes), out))
    return [int(x) for x in out]


def _key32(key):
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("a sampling key is 32 bytes")
    return key


def keyed_small_host(key, nonce, n, count):
    """Host twin of Context.keyed_small (the keyed sampling spec): no context, no GPU.  int8 [count][3][n]."""
    out = np.zeros((count, 3, n), dtype=np.int8)
    _chk(lib().abc_hip_keyed_small_host(_key32(key), nonce % 2 ** 64, n, count, out.ctypes.data_as(C.c_void_p)))
    return out


class DeviceBuffer:
    """A device allocation owned through the C ABI."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _chk(lib().abc_hip_malloc(ctx.h, C.byref(p), C.c_size_t(self.nbytes)))
        self.ptr = p

    def free(self):
        if self.ptr is not None and self.ctx.h:
            lib().abc_hip_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One abc_hip_ctx: parameters, device tables and keys on one GPU."""

    def __init__(self, scheme, n, primes, plain_modulus=0, device=0):
        self.scheme, self.n = scheme, n
        self.logn = n.bit_length() - 1
        self.primes = list(primes)
        self.K, self.L = len(primes), len(primes) - 1
        self.t = plain_modulus
        arr = (C.c_uint64 * len(primes))(*primes)
        h = C.c_void_p()
        _chk(lib().abc_hip_ctx_create(scheme, self.logn, arr, len(primes), C.c_uint64(plain_modulus), device, C.byref(h)))
        self.h = h

    @classmethod
    def bfv_default(cls, n, device=0):
        """The parameters SealCiphertextFactory::setupSealContext picks (SealCiphertextFactory.cpp:72-100)."""
        return cls(BFV, n, default_bfv_primes(n), plain_modulus_batching(n, 20), device)

    def close(self):
        if getattr(self, "h", None):
            lib().abc_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory ----
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(self, arr.nbytes)
        _chk(lib().abc_hip_memcpy_h2d(self.h, buf.ptr, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)))
        return buf

    def download(self, buf, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= buf.nbytes
        _chk(lib().abc_hip_memcpy_d2h(self.h, out.ctypes.data_as(C.c_void_p), buf.ptr, C.c_size_t(out.nbytes)))
        return out

    def sync(self):
        _chk(lib().abc_hip_sync(self.h))

    def trim(self):
        _chk(lib().abc_hip_trim(self.h))

    def cached_bytes(self):
        return int(lib().abc_hip_cached_bytes(self.h))

    def reload_env(self):
        _chk(lib().abc_hip_ctx_reload_env(self.h))

    ROUTE_OPS = {"mul_relin": 0, "keyswitch": 1, "relinearize": 1, "rotate": 2, "rescale": 3, "multiply": 4, "rotate_add": 5,
                 "rotate_mac_plain": 7, "multiply_plain_rescale": 10, "mul_sum_relin": 12, "diag_matvec_bsgs": 13,
                 "bfv_plain_sum": 14, "bfv_matvec_bsgs": 15, "plain_sum_rescale": 16, "diag_matvec_bsgs_rescale": 17,
                 "const_sum_rescale": 18, "poly_eval": 19}

    def route(self, op, nl, count=1, in_place=False):
        """the kernel sequence such a call takes, as the string of abc_route.hpp's formatter"""
        buf = C.create_string_buffer(192)
        _chk(lib().abc_hip_route(self.h, self.ROUTE_OPS.get(op, op), nl, count, int(in_place), buf, len(buf)))
        return buf.value.decode()

    def held_buffers(self):
        """device buffers (scratch arenas, replaced keys) held back for live recorded circuits; -1 from a library without the count"""
        return int(lib().abc_hip_ctx_info(self.h, 6))

    def set_stream(self, stream_ptr):
        _chk(lib().abc_hip_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- keys ----
    def keygen(self, seed=None):
        """seed=None: OS-keyed ChaCha20 (deployment); an integer: the reproducible test sampling spec shared with the oracle"""
        if seed is None:
            _chk(lib().abc_hip_keygen_secure(self.h))
        else:
            _chk(lib().abc_hip_keygen(self.h, C.c_uint64(seed)))

    def keygen_keyed(self, key_sec, key_pub):
        """the keyed sampling spec: key_sec (32 bytes) draws the secret key and the errors, key_pub the published polynomials"""
        _chk(lib().abc_hip_keygen_keyed(self.h, _key32(key_sec), _key32(key_pub)))

    def keyed_small(self, key, nonce, count):
        """the raw draws of encrypt_keyed: int8 [count][3][N] (u | e0 | e1), ciphertext i from stream nonce + i"""
        out = self.alloc(count * 3 * self.n)
        try:
            _chk(lib().abc_hip_keyed_small(self.h, _key32(key), nonce % 2 ** 64, out.ptr, count))
            return self.download(out, (count, 3, self.n), np.int8)
        finally:
            out.free()

    def keyed_uniform(self, key, stream, nkeys):
        """the uniform polynomials of a key: uint64 [nkeys][K][N], limb j modulo q_j, from stream `stream` of `key`"""
        out = self.alloc(nkeys * self.K * self.n * 8)
        try:
            _chk(lib().abc_hip_keyed_uniform(self.h, _key32(key), stream % 2 ** 64, nkeys, out.ptr))
            return self.download(out, (nkeys, self.K, self.n))
        finally:
            out.free()

    def load_keys(self, sk=None, pk=None, relin=None, galois=None):
        def p(a):
            a = np.ascontiguousarray(a, dtype=np.uint64)
            return a, a.ctypes.data_as(u64p)
        if sk is not None:
            a, ptr = p(sk); _chk(lib().abc_hip_load_secret_key(self.h, ptr))
        if pk is not None:
            a, ptr = p(pk); _chk(lib().abc_hip_load_public_key(self.h, ptr))
        if relin is not None:
            a, ptr = p(relin); _chk(lib().abc_hip_load_relin_key(self.h, ptr))
        for elt, key in (galois or {}).items():
            a, ptr = p(key); _chk(lib().abc_hip_load_galois_key(self.h, C.c_uint32(elt), ptr))

    def get_key(self, which, elt=0):
        shape = {"sk": (self.K, self.n), "pk": (2, self.K, self.n)}.get(which, (self.L, 2, self.K, self.n))
        out = np.zeros(shape, dtype=np.uint64)
        ptr = out.ctypes.data_as(u64p)
        if which == "sk":
            _chk(lib().abc_hip_get_secret_key(self.h, ptr))
        elif which == "pk":
            _chk(lib().abc_hip_get_public_key(self.h, ptr))
        elif which == "relin":
            _chk(lib().abc_hip_get_relin_key(self.h, ptr))
        else:
            _chk(lib().abc_hip_get_galois_key(self.h, C.c_uint32(elt), ptr))
        return out

    def galois_elts(self):
        return [int(lib().abc_hip_galois_elt_at(self.h, i)) for i in range(lib().abc_hip_num_galois_keys(self.h))]

    def elt_from_step(self, step):
        return int(lib().abc_hip_galois_elt_from_step(self.h, step))

    # ---- raw device-pointer ops (count = batch) ----
    def op(self, name, *args):
        _chk(getattr(lib(), "abc_hip_" + name)(self.h, *args))

    # ---- numpy convenience: host array in -> device op -> host array out ----
    def _run(self, name, ins, out_shape, *scalars, out_dtype=np.uint64):
        bufs = [self.upload(a) for a in ins]
        out = self.alloc(int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize)
        self.op(name, *[b.ptr for b in bufs], out.ptr, *scalars)
        res = self.download(out, out_shape, out_dtype)
        for b in bufs + [out]:
            b.free()
        return res

    @staticmethod
    def _batch(a, ndim):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return a if a.ndim == ndim + 1 else a[None]

    def add(self, a, b):
        a4, b4 = self._batch(a, 3), self._batch(b, 3)
        r = self._run("add", [a4, b4], a4.shape, a4.shape[1], a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(a) == 4 else r[0]

    def sub(self, a, b):
        a4, b4 = self._batch(a, 3), self._batch(b, 3)
        r = self._run("sub", [a4, b4], a4.shape, a4.shape[1], a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(a) == 4 else r[0]

    def negate(self, a):
        a4 = self._batch(a, 3)
        r = self._run("negate", [a4], a4.shape, a4.shape[1], a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(a) == 4 else r[0]

    def multiply(self, a, b):
        a4, b4 = self._batch(a, 3), self._batch(b, 3)
        shp = (a4.shape[0], 3) + a4.shape[2:]
        r = self._run("multiply", [a4, b4], shp, a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(a) == 4 else r[0]

    def relinearize(self, ct3):
        a4 = self._batch(ct3, 3)
        shp = (a4.shape[0], 2) + a4.shape[2:]
        r = self._run("relinearize", [a4], shp, a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct3) == 4 else r[0]

    def mul_relin(self, a, b):
        a4, b4 = self._batch(a, 3), self._batch(b, 3)
        r = self._run("mul_relin", [a4, b4], a4.shape, a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(a) == 4 else r[0]

    @staticmethod
    def term_pointers(ptrs):
        """a host array of device pointers, as abc_hip_multiply_sum / abc_hip_mul_sum_relin take their terms"""
        ptrs = [(p.value if isinstance(p, C.c_void_p) else p) or 0 for p in ptrs]
        return (C.c_void_p * max(len(ptrs), 1))(*ptrs)

    def _mul_sum(self, name, size, as_, bs, nl, count):
        if len(as_) != len(bs):
            raise ValueError("as many left factors as right factors")
        a4 = [self._batch(a, 3) for a in as_]
        b4 = [self._batch(b, 3) for b in bs]
        if a4:
            count, nl = a4[0].shape[0], a4[0].shape[2]
        elif nl is None:
            raise ValueError("an empty sum needs nl (and count)")
        if any(x.shape != (count, 2, nl, self.n) for x in a4 + b4):
            raise ValueError("every factor is [count][2][nl][N] at one level")
        bufs = {}
        for i, x in enumerate(list(as_) + list(bs)):  # one upload per distinct array: a square or a repeated factor stays one pointer
            if id(x) not in bufs:
                bufs[id(x)] = self.upload((a4 + b4)[i])
        out = self.alloc(max(count * size * nl * self.n * 8, 8))
        try:
            pa = self.term_pointers([bufs[id(x)].ptr for x in as_])
            pb = self.term_pointers([bufs[id(x)].ptr for x in bs])
            self.op(name, pa, pb, len(a4), out.ptr, nl, C.c_size_t(count))
            r = self.download(out, (count, size, nl, self.n))
        finally:
            for b in list(bufs.values()) + [out]:
                b.free()
        return r if not as_ or np.ndim(as_[0]) == 4 else r[0]

    def multiply_sum(self, as_, bs, nl=None, count=1):
        """sum over k of as_[k] (x) bs[k] at size 3 (abc_hip_multiply_sum); nl / count: the shape of an empty sum"""
        return self._mul_sum("multiply_sum", 3, as_, bs, nl, count)

    def mul_sum_relin(self, as_, bs, nl=None, count=1):
        """relinearize(sum over k of as_[k] (x) bs[k]) with one key switch (abc_hip_mul_sum_relin): route("mul_sum_relin") names the sequence"""
        return self._mul_sum("mul_sum_relin", 2, as_, bs, nl, count)

    def rotate(self, ct, steps):
        a4 = self._batch(ct, 3)
        r = self._run("rotate", [a4], a4.shape, a4.shape[2], int(steps), C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct) == 4 else r[0]

    def apply_galois(self, ct, elt):
        a4 = self._batch(ct, 3)
        r = self._run("apply_galois", [a4], a4.shape, a4.shape[2], C.c_uint32(elt), C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct) == 4 else r[0]

    def _hoisted(self, name, ct, ctype, items):
        a4 = self._batch(ct, 3)
        items = [int(x) for x in items]
        arr = (ctype * max(len(items), 1))(*items)
        shp = (len(items),) + a4.shape
        cb = self.upload(a4)
        out = self.alloc(int(np.prod(shp)) * 8)
        try:
            _chk(getattr(lib(), "abc_hip_" + name)(self.h, cb.ptr, out.ptr, a4.shape[2], arr, len(items), a4.shape[0]))
            r = self.download(out, shp)
        finally:
            cb.free(); out.free()
        return r if np.ndim(ct) == 4 else r[:, 0]

    def apply_galois_hoisted(self, ct, elts):
        """several Galois elements of one input (hoisted form): [H][(count,) 2][nl][N], slab r for elts[r].
        Groundwork: slower than H rotate calls until the kernels share the decomposition."""
        return self._hoisted("apply_galois_hoisted", ct, C.c_uint32, elts)

    def rotate_hoisted(self, ct, steps):
        """the same for rotation steps; step 0 is a copy, a step without a key of its own is an error"""
        return self._hoisted("rotate_hoisted", ct, C.c_int, steps)

    def rotate_add(self, ct, addend, steps):
        """addend + rotate(ct, steps) as one call (abc_hip_rotate_add): the add is fused into the key switch where route("rotate_add") says so"""
        a4, b4 = self._batch(ct, 3), self._batch(addend, 3)
        r = self._run("rotate_add", [a4, b4], a4.shape, a4.shape[2], int(steps), C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct) == 4 else r[0]

    def apply_galois_add(self, ct, addend, elt):
        """the same for one Galois element"""
        a4, b4 = self._batch(ct, 3), self._batch(addend, 3)
        r = self._run("apply_galois_add", [a4, b4], a4.shape, a4.shape[2], C.c_uint32(elt), C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct) == 4 else r[0]

    def rotate_sum(self, ct, steps):
        """the rotate-and-sum tree: acc = ct; acc = acc + rotate(acc, s) for each s in steps, in order"""
        a4 = self._batch(ct, 3)
        steps = [int(x) for x in steps]
        arr = (C.c_int * max(len(steps), 1))(*steps)
        r = self._run("rotate_sum", [a4], a4.shape, a4.shape[2], arr, len(steps), C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct) == 4 else r[0]

    def _mac_plain(self, name, ct, plain, addend, arg):
        a4 = self._batch(ct, 3)
        count, nl = a4.shape[0], a4.shape[2]
        plain = np.ascontiguousarray(plain, dtype=np.uint64)
        # [nl][N]: broadcast; [count][rows][N] with rows >= nl: one per ciphertext, rows * N apart (rows encoded for a higher level)
        stride = 0 if plain.ndim == 2 else plain.shape[1] * self.n
        bufs = [self.upload(a4), self.upload(plain)]
        if addend is not None:
            bufs.append(self.upload(self._batch(addend, 3)))
        out = self.alloc(a4.nbytes)
        try:
            self.op(name, bufs[0].ptr, bufs[1].ptr, C.c_size_t(stride), bufs[2].ptr if addend is not None else None, out.ptr, nl, arg,
                    C.c_size_t(count))
            r = self.download(out, a4.shape)
        finally:
            for b in bufs + [out]:
                b.free()
        return r if np.ndim(ct) == 4 else r[0]

    def rotate_mac_plain(self, ct, plain, addend, steps):
        """addend + plain (.) rotate(ct, steps) as one call (abc_hip_rotate_mac_plain), CKKS; addend may be None.  plain: [nl][N] for
        the batch, or [count][rows >= nl][N], one per ciphertext.  Fused into the key switch where route("rotate_mac_plain") says so"""
        return self._mac_plain("rotate_mac_plain", ct, plain, addend, int(steps))

    def apply_galois_mac_plain(self, ct, plain, addend, elt):
        """the same for one Galois element"""
        return self._mac_plain("apply_galois_mac_plain", ct, plain, addend, C.c_uint32(elt))

    def diag_matvec(self, ct, diags, steps):
        """sum over r of diags[r] (.) rotate(ct, steps[r]) (abc_hip_diag_matvec), CKKS; diags [len(steps)][rows >= nl][N], one set for the batch"""
        a4 = self._batch(ct, 3)
        steps = [int(x) for x in steps]
        diags = np.ascontiguousarray(diags, dtype=np.uint64).reshape(len(steps), -1, self.n) if steps else np.zeros((0, a4.shape[2], self.n), np.uint64)
        arr = (C.c_int * max(len(steps), 1))(*steps)
        cb, db = self.upload(a4), self.upload(diags if diags.size else np.zeros(1, dtype=np.uint64))
        out = self.alloc(a4.nbytes)
        try:
            stride = diags.shape[1] * self.n
            self.op("diag_matvec", cb.ptr, db.ptr, C.c_size_t(stride), arr, len(steps), out.ptr, a4.shape[2], C.c_size_t(a4.shape[0]))
            r = self.download(out, a4.shape)
        finally:
            for b in (cb, db, out):
                b.free()
        return r if np.ndim(ct) == 4 else r[0]

    def multiply_plain_sum(self, cts, plains, addend=None, size=2, nl=None, count=1):
        """(addend or 0) + sum over k of plains[k] (.) cts[k] as one call (abc_hip_multiply_plain_sum), CKKS.  cts[k]: [count][size][nl][N]
        (or one ciphertext); plains: all [nl][N], one per term for the batch, or all [count][rows >= nl][N], one per ciphertext.
        size / nl / count: the shape of an empty sum without an addend"""
        return self._plain_sum("multiply_plain_sum", 0, cts, plains, addend, size, nl, count)

    def multiply_plain_sum_rescale(self, cts, plains, addend=None, size=2, nl=None, count=1):
        """rescale((addend or 0) + sum over k of plains[k] (.) cts[k]) as one call (abc_hip_multiply_plain_sum_rescale), CKKS: operands as
        multiply_plain_sum takes them, the result [count][size][nl - 1][N].  The sum of the last terms is formed in the rescale's loads
        where route("plain_sum_rescale") says so"""
        return self._plain_sum("multiply_plain_sum_rescale", 1, cts, plains, addend, size, nl, count)

    def _plain_sum(self, name, drop, cts, plains, addend, size, nl, count):
        if len(cts) != len(plains):
            raise ValueError("as many plaintexts as ciphertexts")
        c4 = [self._batch(x, 3) for x in cts]
        p = [np.ascontiguousarray(x, dtype=np.uint64) for x in plains]
        a4 = None if addend is None else self._batch(addend, 3)
        shape = c4[0].shape if c4 else a4.shape if a4 is not None else (count, size, nl, self.n)
        if shape[2] is None:
            raise ValueError("an empty sum without an addend needs nl (and size, count)")
        if any(x.shape != shape for x in c4 + ([a4] if a4 is not None else [])):
            raise ValueError("every ciphertext is [count][size][nl][N] at one level")
        if any(x.ndim != p[0].ndim or x.shape != p[0].shape for x in p):
            raise ValueError("every plaintext has one form")
        stride = 0 if not p or p[0].ndim == 2 else p[0].shape[1] * self.n
        bufs = {}
        for orig, arr in zip(list(cts) + list(plains), c4 + p):  # one upload per distinct array: a repeated operand stays one pointer
            if id(orig) not in bufs:
                bufs[id(orig)] = self.upload(arr)
        ab = self.upload(a4) if a4 is not None else None
        oshape = (shape[0], shape[1], shape[2] - drop, shape[3])
        out = self.alloc(max(int(np.prod(oshape)) * 8, 8))
        try:
            pc = self.term_pointers([bufs[id(x)].ptr for x in cts])
            pp = self.term_pointers([bufs[id(x)].ptr for x in plains])
            self.op(name, pc, pp, C.c_size_t(stride), len(c4), ab.ptr if ab else None, out.ptr, shape[1], shape[2], C.c_size_t(shape[0]))
            r = self.download(out, oshape)
        finally:
            for b in list(bufs.values()) + [out] + ([ab] if ab else []):
                b.free()
        one = (cts and np.ndim(cts[0]) == 3) or (not cts and addend is not None and np.ndim(addend) == 3)
        return r[0] if one else r

    # ---- scalar constants and polynomial evaluation (CKKS) ----
    def const_words(self, value, scale, nl=None):
        """the words of the constant `value` at `scale` (abc_hip_ckks_const_words): uint64 [nl], round(value * scale) mod q_j; no GPU work"""
        nl = self.L if nl is None else int(nl)
        out = np.zeros(max(nl, 1), dtype=np.uint64)
        _chk(lib().abc_hip_ckks_const_words(self.h, float(value), float(scale), nl, out.ctypes.data_as(u64p)))
        return out[:nl]

    @staticmethod
    def const_sum_args(weights, const, ct_nl, n_terms, nl):
        """the host operands of abc_hip_multiply_const_sum as ctypes values: (h_ct_nl or None, h_weights, h_const or None); keep the
        returned arrays alive across the call"""
        w = np.ascontiguousarray(weights, dtype=np.uint64).reshape(n_terms, nl) if n_terms else np.zeros((1, max(nl, 1)), dtype=np.uint64)
        k = None if const is None else np.ascontiguousarray(const, dtype=np.uint64).reshape(nl)
        l = None if ct_nl is None else (C.c_int * max(n_terms, 1))(*[int(x) for x in ct_nl])
        return l, w, k

    def _const_sum(self, name, drop, cts, weights, const, addend, size, nl, count):
        c4 = [self._batch(x, 3) for x in cts]
        a4 = None if addend is None else self._batch(addend, 3)
        if nl is None:
            nl = a4.shape[2] if a4 is not None else min(x.shape[2] for x in c4) if c4 else None
        if nl is None:
            raise ValueError("an empty sum without an addend needs nl (and size, count)")
        first = c4[0] if c4 else a4
        if first is not None:
            count, size = first.shape[0], first.shape[1]
        if any(x.shape[:2] != (count, size) or x.shape[3] != self.n for x in c4) or (a4 is not None and a4.shape != (count, size, nl, self.n)):
            raise ValueError("every ciphertext is [count][size][its level][N], the addend at nl")
        ct_nl = [x.shape[2] for x in c4]
        l, w, k = self.const_sum_args(weights, const, ct_nl, len(c4), nl)
        bufs = {}
        for orig, arr in zip(cts, c4):  # one upload per distinct array: a repeated operand stays one pointer
            if id(orig) not in bufs:
                bufs[id(orig)] = self.upload(arr)
        ab = self.upload(a4) if a4 is not None else None
        oshape = (count, size, nl - drop, self.n)
        out = self.alloc(max(int(np.prod(oshape)) * 8, 8))
        try:
            pc = self.term_pointers([bufs[id(x)].ptr for x in cts])
            self.op(name, pc, l, w.ctypes.data_as(u64p), len(c4), None if k is None else k.ctypes.data_as(u64p), ab.ptr if ab else None, out.ptr,
                    size, nl, C.c_size_t(count))
            r = self.download(out, oshape)
        finally:
            for b in list(bufs.values()) + [out] + ([ab] if ab else []):
                b.free()
        one = (cts and np.ndim(cts[0]) == 3) or (not cts and addend is not None and np.ndim(addend) == 3)
        return r[0] if one else r

    def multiply_const_sum(self, cts, weights, const=None, addend=None, size=2, nl=None, count=1):
        """(addend or 0) + const (component 0) + sum over k of weights[k] * cts[k] as one call (abc_hip_multiply_const_sum), CKKS.  cts[k]:
        [count][size][its own level >= nl][N] (or one ciphertext), its first nl limbs read; weights [K][nl] and const [nl]: words as
        const_words makes them.  nl: the lowest level among the terms unless given; size / nl / count: the shape of an empty sum"""
        return self._const_sum("multiply_const_sum", 0, cts, weights, const, addend, size, nl, count)

    def multiply_const_sum_rescale(self, cts, weights, const=None, addend=None, size=2, nl=None, count=1):
        """rescale(multiply_const_sum(...)) as one call (abc_hip_multiply_const_sum_rescale): the result [count][size][nl - 1][N]"""
        return self._const_sum("multiply_const_sum_rescale", 1, cts, weights, const, addend, size, nl, count)

    def multiply_const(self, ct, value, scale):
        """ct times the constant `value` at `scale`: the K = 1 form of multiply_const_sum (no encode, no plaintext); the result's scale is
        the ciphertext's times `scale`"""
        nl = np.shape(ct)[-2]
        return self.multiply_const_sum([ct], [self.const_words(value, scale, nl)], nl=nl)

    def add_const(self, ct, value, scale):
        """ct plus the constant `value` at `scale` (the ciphertext's own): the K = 0 form of multiply_const_sum, component 0 only"""
        nl = np.shape(ct)[-2]
        return self.multiply_const_sum([], None, const=self.const_words(value, scale, nl), addend=ct, nl=nl)

    @staticmethod
    def poly_eval_depth(degree):
        """levels a polynomial of this degree consumes (abc_hip_ckks_poly_eval_depth): ceil(log2 degree) + 1"""
        d = int(lib().abc_hip_ckks_poly_eval_depth(int(degree)))
        if d < 0:
            raise AbcHipError(lib().abc_hip_last_error().decode())
        return d

    def poly_eval(self, x, x_scale, coeffs, out_scale):
        """c_0 + c_1 x + ... + c_d x^d on x [count][2][nl][N] (or one ciphertext) at x_scale, by the fixed sequence of
        abc_hip_ckks_poly_eval: the result [count][2][nl - poly_eval_depth(d)][N] at out_scale"""
        a4 = self._batch(x, 3)
        count, _, nl, _ = a4.shape
        co = (C.c_double * max(len(coeffs), 1))(*[float(v) for v in coeffs])
        degree = len(coeffs) - 1
        onl = nl - (self.poly_eval_depth(degree) if degree >= 1 else 1)
        xb = self.upload(a4)
        out = self.alloc(max(count * 2 * max(onl, 0) * self.n * 8, 8))
        try:
            self.op("ckks_poly_eval", xb.ptr, C.c_double(x_scale), co, degree, C.c_double(out_scale), out.ptr, nl, C.c_size_t(count))
            r = self.download(out, (count, 2, onl, self.n))
        finally:
            xb.free(); out.free()
        return r if np.ndim(x) == 4 else r[0]

    def rotate_plain(self, plain, steps):
        """the slot rotation of CKKS plaintexts [rows][nl][N] (or [nl][N]) in NTT form (abc_hip_rotate_plain): no key, any sign of steps"""
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        p3 = p if p.ndim == 3 else p[None]
        r = self._run("rotate_plain", [p3], p3.shape, p3.shape[1], int(steps), C.c_size_t(p3.shape[0]))
        return r if p.ndim == 3 else r[0]

    def bsgs_diagonals(self, diags, baby, giant):
        """the rows abc_hip_diag_matvec_bsgs takes, from plain diagonals: diags[j * len(baby) + i] is the encoded diagonal of step
        giant[j] + baby[i], [rows][N] each; row (j, i) of the result is rotate_plain(that, -giant[j])"""
        d = np.ascontiguousarray(diags, dtype=np.uint64)
        d = d.reshape(len(giant), len(baby), -1, self.n)
        out = np.empty_like(d)
        for j, g in enumerate(giant):
            if len(baby):
                out[j] = self.rotate_plain(d[j], -int(g))
        return out.reshape(len(giant) * len(baby), -1, self.n)

    def diag_matvec_bsgs(self, ct, bsgs_diags, baby, giant):
        """sum over j of rotate(sum over i of bsgs_diags[j * len(baby) + i] (.) rotate(ct, baby[i]), giant[j]) (abc_hip_diag_matvec_bsgs),
        CKKS; bsgs_diags [len(giant) * len(baby)][rows >= nl][N] as bsgs_diagonals makes them, one set for the batch"""
        return self._matvec_bsgs("diag_matvec_bsgs", 0, ct, bsgs_diags, baby, giant)

    def diag_matvec_bsgs_rescale(self, ct, bsgs_diags, baby, giant):
        """the same with every inner sum rescaled before its giant rotation (abc_hip_diag_matvec_bsgs_rescale): the giant steps' key
        switches run at nl - 1 limbs and the result, [count][2][nl - 1][N], arrives rescaled"""
        return self._matvec_bsgs("diag_matvec_bsgs_rescale", 1, ct, bsgs_diags, baby, giant)

    def _matvec_bsgs(self, name, drop, ct, bsgs_diags, baby, giant):
        a4 = self._batch(ct, 3)
        baby, giant = [int(x) for x in baby], [int(x) for x in giant]
        rows = len(baby) * len(giant)
        d = np.ascontiguousarray(bsgs_diags, dtype=np.uint64).reshape(rows, -1, self.n) if rows else np.zeros((0, a4.shape[2], self.n), np.uint64)
        ab, ag = (C.c_int * max(len(baby), 1))(*baby), (C.c_int * max(len(giant), 1))(*giant)
        cb, db = self.upload(a4), self.upload(d if d.size else np.zeros(1, dtype=np.uint64))
        oshape = (a4.shape[0], 2, a4.shape[2] - drop, self.n)
        out = self.alloc(max(int(np.prod(oshape)) * 8, 8))
        try:
            self.op(name, cb.ptr, db.ptr, C.c_size_t(d.shape[1] * self.n), ab, len(baby), ag, len(giant), out.ptr, a4.shape[2],
                    C.c_size_t(a4.shape[0]))
            r = self.download(out, oshape)
        finally:
            for b in (cb, db, out):
                b.free()
        return r if np.ndim(ct) == 4 else r[0]

    # ---- BFV: plaintext-weighted sums with one inverse transform ----
    CT_COEFF, CT_NTT = 0, 1

    def bfv_plain_to_ntt(self, plain):
        """BFV plaintexts [rows][N] (or [N]) mod t -> [rows][L][N] lifted and in NTT form (abc_hip_bfv_plain_to_ntt)"""
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        p2 = p.reshape(-1, self.n)
        shape = (p2.shape[0], self.L, self.n)
        r = self._run("bfv_plain_to_ntt", [p2], shape, C.c_size_t(p2.shape[0])) if p2.shape[0] else np.zeros(shape, np.uint64)
        return r[0] if p.ndim == 1 else r

    def bfv_multiply_plain_sum(self, cts, plains_ntt, addend=None, size=2, count=1, ct_form=0):
        """(addend or 0) + sum over k of plains_ntt[k] * cts[k] with one inverse transform (abc_hip_bfv_multiply_plain_sum), BFV.
        cts[k]: [count][size][L][N] (or one ciphertext) in the form ct_form says; plains_ntt as bfv_plain_to_ntt makes them: all
        [L][N], one per term for the batch, or all [count][L][N], one per ciphertext.  cts and plains_ntt are LISTS (or tuples) of
        arrays: an array that appears twice in them is uploaded once and stays one pointer.  size / count: the shape of an empty sum
        without an addend"""
        cts, plains_ntt = list(cts), list(plains_ntt)  # held for the call: the de-duplication below goes by object identity
        if len(cts) != len(plains_ntt):
            raise ValueError("as many plaintexts as ciphertexts")
        c4 = [self._batch(x, 3) for x in cts]
        p = [np.ascontiguousarray(x, dtype=np.uint64) for x in plains_ntt]
        a4 = None if addend is None else self._batch(addend, 3)
        shape = c4[0].shape if c4 else a4.shape if a4 is not None else (count, size, self.L, self.n)
        if any(x.shape != shape for x in c4 + ([a4] if a4 is not None else [])):
            raise ValueError("every ciphertext is [count][size][L][N]")
        if any(x.shape != p[0].shape for x in p):
            raise ValueError("every plaintext has one form")
        stride = 0 if not p or p[0].ndim == 2 else self.L * self.n
        bufs = {}
        for orig, arr in zip(list(cts) + list(plains_ntt), c4 + p):  # one upload per distinct array: a repeated operand stays one pointer
            if id(orig) not in bufs:
                bufs[id(orig)] = self.upload(arr)
        ab = self.upload(a4) if a4 is not None else None
        out = self.alloc(max(int(np.prod(shape)) * 8, 8))
        try:
            pc = self.term_pointers([bufs[id(x)].ptr for x in cts])
            pp = self.term_pointers([bufs[id(x)].ptr for x in plains_ntt])
            self.op("bfv_multiply_plain_sum", pc, int(ct_form), pp, C.c_size_t(stride), len(c4), ab.ptr if ab else None, out.ptr, shape[1],
                    C.c_size_t(shape[0]))
            r = self.download(out, shape)
        finally:
            for b in list(bufs.values()) + [out] + ([ab] if ab else []):
                b.free()
        one = (len(cts) > 0 and np.ndim(cts[0]) == 3) or (len(cts) == 0 and addend is not None and np.ndim(addend) == 3)
        return r[0] if one else r

    def bfv_bsgs_diagonals(self, diags_cleartext, baby, giant):
        """the rows abc_hip_bfv_diag_matvec_bsgs takes, from cleartext diagonals: diags_cleartext[j * len(baby) + i] holds the N slot
        values of the diagonal of step giant[j] + baby[i]; each half-row is rolled by -giant[j], then batch_encode, then
        bfv_plain_to_ntt.  [len(giant) * len(baby)][L][N]"""
        rows = len(baby) * len(giant)
        if not rows:
            return np.zeros((0, self.L, self.n), dtype=np.uint64)
        d = np.ascontiguousarray(diags_cleartext, dtype=np.int64).reshape(len(giant), len(baby), 2, self.n // 2)
        rolled = np.stack([np.roll(d[j], int(g), axis=2) for j, g in enumerate(giant)])  # roll right by g: the slots of rotate(., -g)
        return self.bfv_plain_to_ntt(self.batch_encode(rolled.reshape(rows, self.n)))

    def bfv_diag_matvec_bsgs(self, ct, bsgs_diags_ntt, baby, giant):
        """sum over j of rotate(sum over i of bsgs_diags_ntt[j * len(baby) + i] * rotate(ct, baby[i]), giant[j])
        (abc_hip_bfv_diag_matvec_bsgs), BFV; bsgs_diags_ntt [len(giant) * len(baby)][L][N] as bfv_bsgs_diagonals makes them"""
        a4 = self._batch(ct, 3)
        baby, giant = [int(x) for x in baby], [int(x) for x in giant]
        rows = len(baby) * len(giant)
        d = np.ascontiguousarray(bsgs_diags_ntt, dtype=np.uint64).reshape(rows, self.L, self.n) if rows else np.zeros((0, self.L, self.n), np.uint64)
        ab, ag = (C.c_int * max(len(baby), 1))(*baby), (C.c_int * max(len(giant), 1))(*giant)
        cb, db = self.upload(a4), self.upload(d if d.size else np.zeros(1, dtype=np.uint64))
        out = self.alloc(a4.nbytes)
        try:
            self.op("bfv_diag_matvec_bsgs", cb.ptr, db.ptr, C.c_size_t(self.L * self.n), ab, len(baby), ag, len(giant), out.ptr,
                    C.c_size_t(a4.shape[0]))
            r = self.download(out, a4.shape)
        finally:
            for b in (cb, db, out):
                b.free()
        return r if np.ndim(ct) == 4 else r[0]

    def _plain_op(self, name, ct, plain):
        a4 = self._batch(ct, 3)
        plain = np.ascontiguousarray(plain, dtype=np.uint64)
        per = self.n if self.scheme == BFV else a4.shape[2] * self.n
        stride = per if plain.size == a4.shape[0] * per and a4.shape[0] > 1 else 0
        if a4.shape[0] == 1:
            stride = 0
        ctb, plb = self.upload(a4), self.upload(plain)
        out = self.alloc(a4.nbytes)
        self.op(name, ctb.ptr, plb.ptr, C.c_size_t(stride), out.ptr, a4.shape[1], a4.shape[2], C.c_size_t(a4.shape[0]))
        r = self.download(out, a4.shape)
        for b in (ctb, plb, out):
            b.free()
        return r if np.ndim(ct) == 4 else r[0]

    def multiply_plain(self, ct, plain):
        return self._plain_op("multiply_plain", ct, plain)

    def add_plain(self, ct, plain):
        return self._plain_op("add_plain", ct, plain)

    def sub_plain(self, ct, plain):
        return self._plain_op("sub_plain", ct, plain)

    def rescale(self, ct):
        a4 = self._batch(ct, 3)
        shp = (a4.shape[0], a4.shape[1], a4.shape[2] - 1, self.n)
        r = self._run("rescale", [a4], shp, a4.shape[1], a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct) == 4 else r[0]

    def multiply_plain_rescale(self, ct, plain):
        """rescale(ct (.) plain) as one call (abc_hip_multiply_plain_rescale), CKKS.  plain: [nl][N] for the batch, or
        [count][rows >= nl][N], one per ciphertext.  The product is formed in the rescale's loads where route("multiply_plain_rescale") says so"""
        a4 = self._batch(ct, 3)
        count, size, nl = a4.shape[:3]
        plain = np.ascontiguousarray(plain, dtype=np.uint64)
        stride = 0 if plain.ndim == 2 else plain.shape[1] * self.n
        shp = (count, size, nl - 1, self.n)
        bufs = [self.upload(a4), self.upload(plain), self.alloc(max(int(np.prod(shp)), 1) * 8)]
        try:
            self.op("multiply_plain_rescale", bufs[0].ptr, bufs[1].ptr, C.c_size_t(stride), bufs[2].ptr, size, nl, C.c_size_t(count))
            r = self.download(bufs[2], shp)
        finally:
            for b in bufs:
                b.free()
        return r if np.ndim(ct) == 4 else r[0]

    def mod_switch(self, ct):
        a4 = self._batch(ct, 3)
        shp = (a4.shape[0], a4.shape[1], a4.shape[2] - 1, self.n)
        r = self._run("mod_switch", [a4], shp, a4.shape[1], a4.shape[2], C.c_size_t(a4.shape[0]))
        return r if np.ndim(ct) == 4 else r[0]

    def keyswitch(self, target, key_kind):
        t3 = self._batch(target, 2)
        shp = (t3.shape[0], 2) + t3.shape[1:]
        tb = self.upload(t3)
        out = self.alloc(int(np.prod(shp)) * 8)
        self.op("keyswitch", tb.ptr, C.c_uint32(key_kind), out.ptr, t3.shape[1], C.c_size_t(t3.shape[0]))
        r = self.download(out, shp)
        tb.free(); out.free()
        return r if np.ndim(target) == 3 else r[0]

    def ntt(self, data, kind, index, inverse=False):
        d = np.ascontiguousarray(data, dtype=np.uint64)
        d2 = d.reshape(-1, self.n)
        buf = self.upload(d2)
        self.op("ntt_inverse" if inverse else "ntt_forward", buf.ptr, kind, index, C.c_size_t(d2.shape[0]))
        r = self.download(buf, d2.shape).reshape(d.shape)
        buf.free()
        return r

    def ntt_limbs(self, data, inverse=False):
        """[polys][nl][N] coefficient form <-> NTT form at a data level (limb j modulo q_j)."""
        d = np.ascontiguousarray(data, dtype=np.uint64)
        d3 = d.reshape(-1, d.shape[-2], self.n)
        buf = self.upload(d3)
        self.op("ntt_limbs", buf.ptr, d3.shape[1], C.c_size_t(d3.shape[0]), 1 if inverse else 0)
        r = self.download(buf, d3.shape).reshape(d.shape)
        buf.free()
        return r

    def batch_encode(self, values):
        v = np.ascontiguousarray(values, dtype=np.int64).reshape(-1, self.n)
        vb = self.upload(v)
        out = self.alloc(v.nbytes)
        self.op("batch_encode", vb.ptr, out.ptr, C.c_size_t(v.shape[0]))
        r = self.download(out, v.shape)
        vb.free(); out.free()
        return r if np.ndim(values) == 2 else r[0]

    def batch_decode(self, plain):
        p = np.ascontiguousarray(plain, dtype=np.uint64).reshape(-1, self.n)
        pb = self.upload(p)
        out = self.alloc(p.nbytes)
        self.op("batch_decode", pb.ptr, out.ptr, C.c_size_t(p.shape[0]))
        r = self.download(out, p.shape, np.int64)
        pb.free(); out.free()
        return r if np.ndim(plain) == 2 else r[0]

    def ckks_encode(self, values, scale, nl=None):
        """CKKS slots -> NTT-form plaintext residues on the device: values real or complex, [count][<= N/2] or one row; the
        slots beyond a row's length are zero.  Returns uint64 [count][nl][N] (or [nl][N] for one row)."""
        v = np.asarray(values)
        rows = v.reshape(-1, v.shape[-1]) if v.ndim else v.reshape(1, 1)
        nl = self.L if nl is None else int(nl)
        count, vpr = rows.shape
        re = np.ascontiguousarray(rows.real, dtype=np.float64)
        im = np.ascontiguousarray(rows.imag, dtype=np.float64) if np.iscomplexobj(rows) else None
        bufs = [self.upload(re)] + ([self.upload(im)] if im is not None else [])
        out = self.alloc(count * max(nl, 0) * self.n * 8 or 8)
        try:
            self.op("ckks_encode", bufs[0].ptr, bufs[1].ptr if im is not None else None, C.c_size_t(vpr), C.c_double(scale), nl,
                    out.ptr, C.c_size_t(count))
            r = self.download(out, (count, nl, self.n))
        finally:
            for b in bufs + [out]:
                b.free()
        return r if v.ndim == 2 else r[0]

    def ckks_decode(self, plain, scale):
        """NTT-form plaintext residues [count][nl][N] (or [nl][N]) -> complex slot values [count][N/2] (or [N/2]), divided by scale."""
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        p3 = p if p.ndim == 3 else p[None]
        count, nl = p3.shape[0], p3.shape[1]
        slots = self.n // 2
        pb = self.upload(p3)
        re, im = self.alloc(count * slots * 8), self.alloc(count * slots * 8)
        try:
            self.op("ckks_decode", pb.ptr, nl, C.c_double(scale), re.ptr, im.ptr, C.c_size_t(count))
            r = self.download(re, (count, slots), np.float64) + 1j * self.download(im, (count, slots), np.float64)
        finally:
            for b in (pb, re, im):
                b.free()
        return r if p.ndim == 3 else r[0]

    def encrypt(self, plain, seed=None):
        per = (self.n,) if self.scheme == BFV else (self.L, self.n)
        p = np.ascontiguousarray(plain, dtype=np.uint64).reshape((-1,) + per)
        pb = self.upload(p)
        shp = (p.shape[0], 2, self.L, self.n)
        out = self.alloc(int(np.prod(shp)) * 8)
        if seed is None:
            self.op("encrypt_secure", pb.ptr, out.ptr, C.c_size_t(p.shape[0]))
        else:
            self.op("encrypt", pb.ptr, C.c_uint64(seed), out.ptr, C.c_size_t(p.shape[0]))
        r = self.download(out, shp)
        pb.free(); out.free()
        return r if np.ndim(plain) == len(per) + 1 else r[0]

    def encrypt_keyed(self, plain, key, nonce=0):
        """the keyed sampling spec: ciphertext i of the batch draws from stream nonce + i of `key` (32 bytes); never reuse a pair"""
        per = (self.n,) if self.scheme == BFV else (self.L, self.n)
        p = np.ascontiguousarray(plain, dtype=np.uint64).reshape((-1,) + per)
        pb = self.upload(p)
        shp = (p.shape[0], 2, self.L, self.n)
        out = self.alloc(int(np.prod(shp)) * 8)
        try:
            _chk(lib().abc_hip_encrypt_keyed(self.h, pb.ptr, _key32(key), nonce % 2 ** 64, out.ptr, p.shape[0]))
            r = self.download(out, shp)
        finally:
            pb.free(); out.free()
        return r if np.ndim(plain) == len(per) + 1 else r[0]

    def decrypt(self, ct):
        a4 = self._batch(ct, 3)
        cb = self.upload(a4)
        shp = (a4.shape[0], self.n) if self.scheme == BFV else (a4.shape[0], a4.shape[2], self.n)
        out = self.alloc(int(np.prod(shp)) * 8)
        self.op("decrypt", cb.ptr, a4.shape[1], a4.shape[2], out.ptr, C.c_size_t(a4.shape[0]))
        r = self.download(out, shp)
        cb.free(); out.free()
        return r if np.ndim(ct) == 4 else r[0]

    def noise_budget(self, ct):
        """Invariant noise budget in bits of BFV ciphertexts [size][L][N] (-> int) or [count][size][L][N] (-> np.int32 array),
        computed on the device: only the budgets come back."""
        a4 = self._batch(ct, 3)
        cb = self.upload(a4)
        out = np.zeros(a4.shape[0], dtype=np.int32)
        try:
            self.op("noise_budget", cb.ptr, a4.shape[1], a4.shape[2], out.ctypes.data_as(C.POINTER(C.c_int)), C.c_size_t(a4.shape[0]))
        finally:
            cb.free()
        return out if np.ndim(ct) == 4 else int(out[0])

    # ---- HIP-graph capture of an op sequence ----
    def graph_begin(self):
        _chk(lib().abc_hip_graph_begin(self.h))

    def graph_end(self):
        g = C.c_void_p()
        _chk(lib().abc_hip_graph_end(self.h, C.byref(g)))
        return g

    def graph_launch(self, g):
        _chk(lib().abc_hip_graph_launch(self.h, g))

    def graph_destroy(self, g):
        _chk(lib().abc_hip_graph_destroy(self.h, g))

    def microbench(self, which, iters):
        ms = C.c_double()
        _chk(lib().abc_hip_microbench(self.h, which, iters, C.byref(ms)))
        return ms.value

    def timer_start(self):
        _chk(lib().abc_hip_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        _chk(lib().abc_hip_timer_stop(self.h, C.byref(ms)))
        return ms.value
