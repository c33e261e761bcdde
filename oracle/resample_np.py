"""Plain restatement of the device-drawn bootstrap resample (TEST INFRASTRUCTURE ONLY).

Written from the Philox paper (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
1, 2, 3", SC'11, section 3.3 and table 2) and from the contract of oem_bootstrap_weights
(include/oarfish_em.h), not from the kernel.  philox4x32-10 is stated twice,
once on Python ints one block at a time and once on NumPy u64 lanes, so that the two forms check
each other (tests/test_resample_reference.py also holds both to the Random123 known answers).

The contract.  Replica `replica` of seed `seed` over a store of n_global reads is n_global draws
from Uniform[0, n_global) (bootstrap.rs:7-16), in multiplicity form:

  counter block q < ceil(n_global / 2):  (q & 0xffffffff, q >> 32, replica, 0x6f656d62 "oemb")
  key:                                   (seed & 0xffffffff, seed >> 32)
  draw 2q   = (out[0] << 32) | out[1],   draw 2q+1 = (out[2] << 32) | out[3]
  draws with index >= n_global do not exist (the second half of the last block of an odd store)
  read index of a draw r = (r * n_global) >> 64

and a row shard [local_off, local_off + n_local) keeps the histogram of the indices it owns.
"""
from __future__ import annotations

import numpy as np

# SC'11 table 2 / section 3.3: the round multipliers and the Weyl key increments of philox4x32
PHILOX_M0 = 0xD2511F53
PHILOX_M1 = 0xCD9E8D57
PHILOX_W0 = 0x9E3779B9   # golden ratio
PHILOX_W1 = 0xBB67AE85   # sqrt(3) - 1
DOMAIN_TAG = 0x6F656D62  # "oemb": counter word 3 of the bootstrap stream
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def philox4x32_10(counter, key):
    """Scalar form on Python ints: counter (4 words), key (2 words) -> 4 output words.
    One round: (c0, c1, c2, c3) -> (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0));
    the key is bumped by the Weyl constants between rounds (before rounds 2..10)."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for rnd in range(10):
        if rnd:
            k0 = (k0 + PHILOX_W0) & _M32
            k1 = (k1 + PHILOX_W1) & _M32
        p0 = PHILOX_M0 * c0
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
    return c0, c1, c2, c3


def philox4x32_10_np(counter, key):
    """Vectorised form: counter[..., 4] and key[..., 2] of 32-bit words (broadcast against each
    other) -> uint64[..., 4] holding the 32-bit output words.  A 32x32 product fits a u64 lane."""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    m32, s32 = np.uint64(_M32), np.uint64(32)
    c = [np.broadcast_to(counter[..., i] & m32, shape) for i in range(4)]
    k = [np.broadcast_to(key[..., i] & m32, shape) for i in range(2)]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(PHILOX_W0)) & m32, (k[1] + np.uint64(PHILOX_W1)) & m32]
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
    return np.stack(c, axis=-1)


def mulhi64(a, n):
    """High 64 bits of the 128-bit product a * n, a: uint64 array, n: one integer < 2^64.
    Schoolbook on 32-bit halves; no partial sum exceeds 2^64 - 1."""
    a = np.asarray(a, dtype=np.uint64)
    n = int(n)
    if not 0 <= n <= _M64:
        raise ValueError("n must fit 64 bits")
    m32, s32 = np.uint64(_M32), np.uint64(32)
    a_lo, a_hi = a & m32, a >> s32
    n_lo, n_hi = np.uint64(n & _M32), np.uint64(n >> 32)
    ll = a_lo * n_lo
    lh = a_lo * n_hi
    hl = a_hi * n_lo
    hh = a_hi * n_hi
    mid = (ll >> s32) + (lh & m32) + (hl & m32)   # < 3 * 2^32
    return hh + (lh >> s32) + (hl >> s32) + (mid >> s32)


_CHUNK = 1 << 20  # counter blocks per vectorised step (bounds the temporaries of a 10 M-read draw)


def bootstrap_weights(n_global, seed, replica, local_off=0, n_local=None):
    """The multiplicities oem_bootstrap_weights(seed, replica) returns on a store holding rows
    [local_off, local_off + n_local) of n_global reads: uint32[n_local]."""
    n_global, seed, replica, local_off = int(n_global), int(seed), int(replica), int(local_off)
    n_local = n_global - local_off if n_local is None else int(n_local)
    if not (0 <= seed <= _M64 and 0 <= replica <= _M32):
        raise ValueError("seed is 64 bits, replica 32 bits")
    if local_off < 0 or n_local < 0 or local_off + n_local > n_global:
        raise ValueError("the shard exceeds the store")
    out = np.zeros(n_local, dtype=np.int64)
    key = np.array([seed & _M32, seed >> 32], dtype=np.uint64)
    n_blocks = (n_global + 1) // 2
    for q0 in range(0, n_blocks, _CHUNK):
        q = np.arange(q0, min(q0 + _CHUNK, n_blocks), dtype=np.uint64)
        ctr = np.empty((len(q), 4), dtype=np.uint64)
        ctr[:, 0] = q & np.uint64(_M32)
        ctr[:, 1] = q >> np.uint64(32)
        ctr[:, 2] = replica
        ctr[:, 3] = DOMAIN_TAG
        o = philox4x32_10_np(ctr, key)
        draws = np.empty(2 * len(q), dtype=np.uint64)          # draw index 2*q0 + position
        draws[0::2] = (o[:, 0] << np.uint64(32)) | o[:, 1]
        draws[1::2] = (o[:, 2] << np.uint64(32)) | o[:, 3]
        draws = draws[:n_global - 2 * q0]                      # the draw past an odd store's end
        idx = mulhi64(draws, n_global).astype(np.int64)
        idx = idx[(idx >= local_off) & (idx < local_off + n_local)] - local_off
        out += np.bincount(idx, minlength=n_local)
    return out.astype(np.uint32)


def bootstrap_weights_scalar(n_global, seed, replica, local_off=0, n_local=None):
    """The same contract, one draw at a time on Python ints (small stores: cross-check of the
    vectorised form)."""
    n_global, seed, replica, local_off = int(n_global), int(seed), int(replica), int(local_off)
    n_local = n_global - local_off if n_local is None else int(n_local)
    out = np.zeros(n_local, dtype=np.uint32)
    for k in range(n_global):
        q, half = divmod(k, 2)
        o = philox4x32_10((q & _M32, q >> 32, replica, DOMAIN_TAG), (seed & _M32, seed >> 32))
        r = (o[2 * half] << 32) | o[2 * half + 1]
        idx = (r * n_global) >> 64
        if local_off <= idx < local_off + n_local:
            out[idx - local_off] += 1
    return out
