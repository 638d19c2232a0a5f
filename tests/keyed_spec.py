"""The keyed sampling spec ("Keyed sampling spec") restated in Python -- TEST INFRASTRUCTURE ONLY.

Written from RFC 8439 (section 2.1 quarter round, 2.3 block function) and the spec text, not from the C++: numpy uint32
arithmetic over many blocks at once for the block function, Python integers for the wide reduction.
"""
import numpy as np

M64 = (1 << 64) - 1
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"


def _rotl(v, k):
    return (v << np.uint32(k)) | (v >> np.uint32(32 - k))


def _quarter_round(x, a, b, c, d):
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 16)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 12)
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 8)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 7)


def blocks(key, stream, first, count):
    """ChaCha20 blocks first .. first + count - 1 of stream `stream`: uint32 [count][16] (the serialised block, word by word)"""
    assert len(key) == 32
    ctr = (np.arange(count, dtype=np.uint64) + np.uint64(first))
    state = [np.full(count, c, dtype=np.uint32) for c in CONSTANTS]
    state += [np.full(count, int.from_bytes(key[4 * i:4 * i + 4], "little"), dtype=np.uint32) for i in range(8)]
    state += [(ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32)]
    state += [np.full(count, stream & 0xFFFFFFFF, dtype=np.uint32), np.full(count, (stream >> 32) & 0xFFFFFFFF, dtype=np.uint32)]
    x = [s.copy() for s in state]
    for _ in range(10):
        _quarter_round(x, 0, 4, 8, 12); _quarter_round(x, 1, 5, 9, 13); _quarter_round(x, 2, 6, 10, 14); _quarter_round(x, 3, 7, 11, 15)
        _quarter_round(x, 0, 5, 10, 15); _quarter_round(x, 1, 6, 11, 12); _quarter_round(x, 2, 7, 8, 13); _quarter_round(x, 3, 4, 9, 14)
    return np.stack([a + b for a, b in zip(x, state)], axis=1)


def words(key, stream, first_word, count):
    """64-bit words first_word .. first_word + count - 1 of a stream: word W is word W mod 8 of block W div 8"""
    b0, b1 = first_word // 8, (first_word + count + 7) // 8
    out = blocks(key, stream & M64, b0, b1 - b0).astype(np.uint64)
    w = (out[:, 0::2] | (out[:, 1::2] << np.uint64(32))).reshape(-1)
    return w[first_word - 8 * b0: first_word - 8 * b0 + count]


def ternary(w):
    return (np.asarray(w, dtype=np.uint64) % np.uint64(3)).astype(np.int8) - np.int8(1)


def _popcount21(v):
    bits = np.unpackbits((v & np.uint64(0x1FFFFF)).astype("<u4").view(np.uint8).reshape(-1, 4), axis=1)
    return bits.sum(axis=1).astype(np.int8)


def cbd(w):
    w = np.asarray(w, dtype=np.uint64)
    return _popcount21(w) - _popcount21(w >> np.uint64(21))


def uniform_q(lo, hi, q):
    return ((int(hi) << 64) + int(lo)) % q


def encrypt_small(key, nonce, n, count):
    """int8 [count][3][n]: u | e0 | e1 of ciphertext i from stream nonce + i (mod 2^64), words x, n + x, 2n + x"""
    out = np.empty((count, 3, n), dtype=np.int8)
    for i in range(count):
        w = words(key, (nonce + i) & M64, 0, 3 * n)
        out[i, 0] = ternary(w[:n])
        out[i, 1] = cbd(w[n:2 * n])
        out[i, 2] = cbd(w[2 * n:])
    return out


def secret(key_sec, n):
    return ternary(words(key_sec, 0, 0, n))


def key_errors(key_sec, stream, n, nkeys):
    """int8 [nkeys][n]: e_i[x] from word i*n + x"""
    return cbd(words(key_sec, stream, 0, nkeys * n)).reshape(nkeys, n)


def key_uniform(key_pub, stream, n, primes, nkeys):
    """uint64 [nkeys][K][n]: a_i[j][x] from words 2t (lo), 2t + 1 (hi), t = (i*K + j)*n + x, reduced mod q_j"""
    K = len(primes)
    w = words(key_pub, stream, 0, 2 * nkeys * K * n).astype(object).reshape(nkeys, K, n, 2)
    wide = (w[..., 1] << 64) + w[..., 0]
    out = np.empty((nkeys, K, n), dtype=np.uint64)
    for j, q in enumerate(primes):
        out[:, j, :] = (wide[:, j, :] % int(q)).astype(np.uint64)
    return out
