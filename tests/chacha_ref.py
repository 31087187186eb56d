"""Plain-Python reference of the engine's device randomness (Randomness): the ChaCha20 block
function, the seeded key expansion, the rejection sampler of k_rng_r and the digit stream of k_rng_digits
(fedtree_amd/csrc/fthe_glue.hip), written from their contract and sharing no code with them.  The GPU tests
build their expected ciphertexts from these draws and Python integers alone (tests/test_gpu_rng_stream.py).

The contract.  A stream is a (key, nonce) pair: rng_key(seed, tweak), the nonce then changed as the table says.
Ciphertext `index` of a call (index0 + its row) owns a fixed range of 64-bit block counters of its stream, so a
draw depends on the index alone: not on the batch size, the chunking or the shard (index0) it was made in.

  k_rng_r       draw_below(): attempt a = 0..63 of index i takes blocks (i * 64 + a) * nblk + b, b < nblk =
                ceil(row_words / 16); the candidate is the first row_words words, little-endian, with every bit
                at or above nbits cleared; the first candidate with 0 < candidate < modulus is the draw; after
                64 failures (probability below 2^-64 when nbits is the modulus's bit length) the draw is 1
  k_rng_digits  digits(): index i, side s take blocks (i * 2 + s) * nb + b, b < nb = ceil(nbytes / 64); the
                exponent is the first nbytes bytes of those blocks, little-endian

  stream                            tweak               nonce change                        kernel
  CRT direct-y, y_p                 0                   none                                k_rng_r, row_words = pq_w
  CRT direct-y, y_q                 0                   nonce XOR 0x7172737475767778        k_rng_r, row_words = pq_w
  public-key r                      0                   none                                k_rng_r, row_words = n_words,
                                                                                            nbits = bits of n
  exact fixed-base, key holder      0x6578616374626173  per (side, base b):                 k_rng_r, row_words = pq_w
                                                        nonce += (3 side + b + 1) << 56
  published-bases public exact      0x7075626c69636273  per base b: nonce += (b + 1) << 56  k_rng_digits, side 0,
                                                                                            two bytes per digit
  fixed_base                        0x6669786564626173  none                                k_rng_digits, side 0 for p
                                                                                            and for the public form,
                                                                                            side 1 for q

pq_w is the word count of the larger prime; in the k_rng_r rows nbits is the bit length of the modulus sampled
(p, q or n), whatever the row width.  Counter and nonce arithmetic is modulo 2^64.
"""
import numpy as np

M64 = (1 << 64) - 1
YQ_XOR = 0x7172737475767778
TWEAK_EXACT = 0x6578616374626173
TWEAK_PUBLIC_EXACT = 0x7075626C69636273
TWEAK_FIXED_BASE = 0x6669786564626173
ATTEMPTS = 64

_CONST = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)        # "expand 32-byte k"


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def _quarter(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key8, counter64, nonce64):
    """The 16 output words of ChaCha20 blocks: words 0-3 the constants, 4-11 the key, 12, 13 the counter (low,
    high), 14, 15 the nonce (low, high); 20 rounds, then the input state added.  counter64: an int or an array
    of ints; returns uint32 of shape (16,) or (len, 16)."""
    ctr = np.atleast_1d(np.asarray(counter64, dtype=np.uint64))
    s = [np.full(ctr.shape, v, dtype=np.uint32) for v in _CONST]
    s += [np.full(ctr.shape, int(v) & 0xFFFFFFFF, dtype=np.uint32) for v in key8]
    s += [(ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32)]
    s += [np.full(ctr.shape, int(nonce64) & 0xFFFFFFFF, dtype=np.uint32),
          np.full(ctr.shape, (int(nonce64) >> 32) & 0xFFFFFFFF, dtype=np.uint32)]
    assert len(s) == 16
    x = [v.copy() for v in s]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
            _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
        out = np.stack([a + b for a, b in zip(x, s)], axis=-1)
    return out[0] if np.ndim(counter64) == 0 else out


def _splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def rng_key(seed, tweak):
    """(key8, nonce64) of a seeded stream: four splitmix64 outputs from state `seed` give the key words (low half
    first), a fifth XOR tweak the nonce."""
    assert 0 < seed <= M64
    s, key = seed, []
    for _ in range(4):
        s, v = _splitmix64(s)
        key += [v & 0xFFFFFFFF, v >> 32]
    s, v = _splitmix64(s)
    return key, v ^ tweak


def _stream_bytes(key, nonce, first_block, nblocks):
    """first_block: array of n block counters -> (n, 64 * nblocks) bytes of blocks first_block + 0 .. nblocks-1"""
    first = np.asarray(first_block, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = (first[:, None] + np.arange(nblocks, dtype=np.uint64)[None, :]).reshape(-1)
    words = np.ascontiguousarray(chacha20_block(key, ctr, nonce).astype("<u4"))
    return words.view(np.uint8).reshape(len(first), nblocks * 64)


def _u64(values):
    return np.array([int(v) & M64 for v in values], dtype=np.uint64)


def draw_below_many(key, nonce, indices, modulus, nbits, row_words):
    """draw_below for a list of indices: ([values], [attempts]); the blocks of one attempt of all the indices
    still undecided are computed together."""
    indices = [int(i) for i in indices]
    assert 0 < nbits <= 32 * row_words
    nblk = (row_words + 15) // 16
    mask = (1 << nbits) - 1
    value, tries = [1] * len(indices), [ATTEMPTS] * len(indices)
    todo = list(range(len(indices)))
    for a in range(ATTEMPTS):
        if not todo:
            break
        rows = _stream_bytes(key, nonce, _u64((indices[j] * 64 + a) * nblk for j in todo), nblk)
        left = []
        for j, row in zip(todo, rows):
            cand = int.from_bytes(row[:4 * row_words].tobytes(), "little") & mask
            if 0 < cand < modulus:
                value[j], tries[j] = cand, a + 1
            else:
                left.append(j)
        todo = left
    return value, tries


def draw_below(key, nonce, index, modulus, nbits, row_words):
    """The rejection sampler: (value, attempts).  attempts counts the candidates drawn, 1..64; after 64 failures
    the value is 1 (and attempts 64)."""
    v, t = draw_below_many(key, nonce, [index], modulus, nbits, row_words)
    return v[0], t[0]


def digits_many(key, nonce, indices, side, nbytes):
    """digits for a list of indices, as ints (little-endian)"""
    nb = (nbytes + 63) // 64
    rows = _stream_bytes(key, nonce, _u64((int(i) * 2 + side) * nb for i in indices), nb)
    return [int.from_bytes(row[:nbytes].tobytes(), "little") for row in rows]


def digits(key, nonce, index, side, nbytes):
    """The nbytes exponent bytes of (index, side), in stream order."""
    nb = (nbytes + 63) // 64
    return _stream_bytes(key, nonce, _u64([(int(index) * 2 + side) * nb]), nb)[0, :nbytes].tobytes()
