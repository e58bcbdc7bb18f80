"""Plain references of the in-kernel exploration noise (csrc/ks_select.h): Philox4x32-10 in numpy integer arithmetic and normal4's
uniforms + Box-Muller in fp64.  Vectorised over arrays of counters."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(c, k):
    """c: four uint32 arrays (or ints), k: two -> four uint32 arrays.  Random123's philox4x32 with 10 rounds: key bumped between rounds."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in c]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK for x in k)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # < 2^64: exact in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return [x.astype(np.uint32) for x in c]


def normal4(seed, step, env):
    """fp64 reference of krsel::normal4: counter (env, step low word, step high word, 0x4b52), key (seed low word, seed high word); the top 24 bits
    of each word -> uniforms (r + 0.5) / 2^24; Box-Muller on the pairs (u0, u1) and (u2, u3).  Returns [..., 4] float64."""
    seed, step, env = (np.asarray(x, dtype=np.uint64) for x in (seed, step, env))
    seed, step, env = np.broadcast_arrays(seed, step, env)
    r = philox4x32_10((env & MASK, step & MASK, step >> np.uint64(32), np.full_like(env, 0x4B52)), (seed & MASK, seed >> np.uint64(32)))
    # the uniforms exactly as the kernel forms them: (r >> 8) + 0.5 in fp32 (words >= 2^23 round to an integer - u = 1 is possible) / 2^24 (exact)
    u = [((x >> np.uint32(8)).astype(np.float32) + np.float32(0.5)).astype(np.float64) / 16777216.0 for x in r]
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a, b = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], -1)
