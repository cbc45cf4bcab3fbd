"""Times wf_grind_seeds (the proof-of-work nonce of the query seed) for every hasher.
  1. calls: 32 fixed seeds, one call per seed and one call for all 32, at three grinding factors; median wall clock per call,
     the answers' spread, and the device time of the search launches (events around every launch).
  2. rate: a search that finds nothing (factor 32 over a fixed range), so that every window is hashed to its end: nonces per
     second = range / device time of the launches, and each window's size and time -- what the window cap is set from.
  3. floor: a call at factor 0 (one window, first nonce).
  4. the CPU's merge_with_int on one thread (the oracle's BLAKE3 through ctypes, call overhead included; hashlib's SHA3).
Compare the rates with the register-only loops of scripts/merkle_bench.hip, keccak_bench.hip, rescue_bench.hip, rescue_jive_bench.hip and griffin_bench.hip run in the
same session.
    python scripts/time_grind.py [hasher ...]     hashers: blake3_256 blake3_192 sha3_256 rp64_256 rpjive64_256 griffin (default: all)"""
import hashlib, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import starkpack_winterfell_amd.capi as capi

HASHERS = {"blake3_256": (capi.BLAKE3, 32), "blake3_192": (capi.BLAKE3, 24), "sha3_256": (capi.SHA3_256, 32),
           "rp64_256": (capi.RP64_256, 32), "rpjive64_256": (capi.RPJIVE64_256, 32), "griffin": (capi.GRIFFINJIVE64_256, 32)}
FACTORS = {"rp64_256": (12, 16, 20), "rpjive64_256": (12, 16, 20), "griffin": (12, 16, 20)}
RATE_RANGE_LOG2 = {"blake3_256": 31, "blake3_192": 31, "sha3_256": 29, "rp64_256": 25, "rpjive64_256": 25, "griffin": 27}
WARMUP, REPEATS = 2, 5


def seeds_for(name, n=32):
    out = []
    for k in range(n):
        s = hashlib.sha256(b"grind seed %d" % k).digest()
        out.append(s[:24] + bytes(8) if name == "blake3_192" else s)
    return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(n, 32)


def launches(ctx):
    """[(mark, ms)] of the last calls; the search launches are the 'grind.window' marks."""
    return [ms for name, ms in ctx.profile_read() if name == "grind.window"]


def timed(fn):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        r = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), r


def main():
    names = sys.argv[1:] or list(HASHERS)
    ctx = capi.Context(0)
    for name in names:
        hasher, db = HASHERS[name]
        ctx.set_hasher(capi.BLAKE3)
        ctx.set_digest_bytes(db)
        ctx.set_hasher(hasher)
        seeds = seeds_for(name)
        print(f"== {name}")
        ms, _ = timed(lambda: ctx.grind(seeds[:1], 0))
        print(f"floor: factor 0, one seed: {ms * 1e3:.1f} us per call (wall, median of {REPEATS})")
        for g in FACTORS.get(name, (16, 20, 24)):
            single, nonces = [], []
            for i in range(len(seeds)):
                ms, (n, _, f) = timed(lambda: ctx.grind(seeds[i:i + 1], g))
                assert f[0] == 1
                single.append(ms)
                nonces.append(int(n[0]))
            batch_ms, (bn, _, bf) = timed(lambda: ctx.grind(seeds, g))
            assert bf.all() and [int(x) for x in bn] == nonces
            ctx.profile_enable(2)
            ctx.grind(seeds, g)
            dev = launches(ctx)
            ctx.profile_enable(0)
            print(f"factor {g}: one seed per call {statistics.median(single):.3f} ms median over {len(seeds)} seeds (min {min(single):.3f}, max "
                  f"{max(single):.3f}); answers 2^{np.log2(min(nonces)):.1f} .. 2^{np.log2(max(nonces)):.1f}, median 2^{np.log2(statistics.median(nonces)):.1f}; "
                  f"32 seeds in one call {batch_ms:.3f} ms ({len(dev)} launches, {sum(dev):.3f} ms on the device)")
        # nothing found: every window is hashed to its end
        lg = RATE_RANGE_LOG2[name]
        rates = []
        for i in range(4):
            ctx.grind(seeds[i:i + 1], 32, 1, 1 << lg)  # warm-up
            ctx.profile_enable(2)
            t0 = time.perf_counter()
            _, _, f = ctx.grind(seeds[i:i + 1], 32, 1, 1 << lg)
            wall = (time.perf_counter() - t0) * 1e3
            dev = launches(ctx)
            ctx.profile_enable(0)
            if f[0]:
                print(f"rate: seed {i} has a factor-32 nonce below 2^{lg}: left out")
                continue
            rates.append((1 << lg) / (sum(dev) * 1e-3))
            print(f"rate: seed {i}, 2^{lg} nonces, nothing found: {len(dev)} launches, {sum(dev):.3f} ms on the device, {wall:.3f} ms wall: "
                  f"{rates[-1] / 1e9:.3f} G nonces/s on the device, {(1 << lg) / wall / 1e6:.3f} G nonces/s by the wall clock")
            if len(rates) == 1:
                print("      windows (ms):", " ".join(f"{x:.3f}" for x in dev[:16]), "..." if len(dev) > 16 else "")
        if rates:
            print(f"rate: median {statistics.median(rates) / 1e9:.3f} G nonces/s")
    ctx.close()

    # the CPU, one thread
    from oracle import oracle as O
    O.build()
    seed = bytes(seeds_for("blake3_256", 1)[0])
    t0 = time.perf_counter()
    n = 200000
    for v in range(n):
        O.merge_with_int(seed, v)
    dt = time.perf_counter() - t0
    print(f"== CPU, one thread: the oracle's BLAKE3 merge_with_int through ctypes {n / dt / 1e6:.3f} M/s ({dt / n * 1e9:.0f} ns per call, call overhead included)")
    t0 = time.perf_counter()
    for v in range(n):
        hashlib.sha3_256(seed + v.to_bytes(8, "little")).digest()
    dt = time.perf_counter() - t0
    print(f"== CPU, one thread: hashlib.sha3_256 of 40 bytes {n / dt / 1e6:.3f} M/s ({dt / n * 1e9:.0f} ns per call)")


if __name__ == "__main__":
    main()
