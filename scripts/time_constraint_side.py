"""Times the constraint side at cfg 2's proof shape (trace 2^20, constraint evaluation domain 2^21, quadratic extension, two
composition columns): wf_constraint_commit_from_tables (one packed trace: a transition column and a single-step assertion
column) and wf_constraint_commit_from_evaluations, wall clock and per-launch device times.
    python scripts/time_constraint_side.py [logR] [log_ce_blowup]

The device-evaluated route next to the host-table one, interleaved round by round on one box:
    python scripts/time_constraint_side.py device <cfg: 2 | 5> [rounds] [program]
  new  wf_constraint_evaluate + wf_constraint_commit_from_device_tables on a resident trace commitment;
  old  wf_commitment_read_lde_strided of the constraint evaluation domain's rows + wf_constraint_commit_from_tables on host
       columns, with NO time charged for the CPU evaluation in between (the columns are prepared outside the clock): a lower
       bound of the route a host had before.
  cfg 2: f64, 2^20 x 8, blowup 8 (programs fib -- memory-bound -- and stress -- ALU-bound); cfg 5: f128, 2^18 x 10, the do_work
  program.  ce blowup 4, quadratic extension.  Also prints the planner's work-group size and LDS bytes, the kernel's device time,
  the bytes it moves and the base-field products it executes per second.

The same comparison for an AIR with an auxiliary segment (wf_constraint_evaluate_aux; old: the read-back of BOTH LDEs):
    python scripts/time_constraint_side.py aux [rounds]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import starkpack_winterfell_amd.capi as capi


def device_route(cfg, rounds, name):
    import ctypes as C
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import cprog_util as U
    import edge_util as E
    field, logR, n_cols = (capi.F64, 20, 8) if cfg == 2 else (capi.F128, 18, 10)
    name = name or ("fib" if cfg == 2 else "do_work")
    ext, logB, lce, n_cols_c = 2, 3, 2, 2
    R, ce, w = 1 << logR, 1 << (logR + lce), capi.ELEM_WORDS[field]
    ctx = capi.Context(0)
    rng = np.random.default_rng(cfg)
    cols = [rng.integers(0, 2**62, size=(R, w) if w > 1 else R, dtype=np.uint64) for _ in range(n_cols)]
    com, _ = ctx.trace_commit_resident(capi.make_params(field, 1, logR, logB, n_cols, 1), cols)
    g = U.build(name, field, ext, rng, ce, 1 << lce, n_cols)
    prog = U.to_capi(capi, g, field, ext)
    one = E.elements(field, [E.ONE[field]])
    gR = E.elements(field, [U.to_mem(field, pow(U.root_of_unity(field, logR), R - 1, U.P[field]))])
    divs = [(R, one, gR)] + [(1, gR, None)] * (len(g.out_regs) - 1)
    p = capi.make_params(field, ext, logR, logB, n_cols_c, 1)
    ev = ctx.constraint_evaluate(com, 0, prog, ext, lce)
    host_cols = [ev.read(j) for j in range(ev.n_columns)]
    ev.close()
    L = capi.load()
    rw = C.c_uint64()
    L.wf_commitment_read_lde(com._h, 0, 0, 0, None, C.byref(rw))
    frame_buf = np.zeros((ce, rw.value, w) if w > 1 else (ce, rw.value), dtype=np.uint64)   # touched: no page faults in the clock
    stride = 1 << (logB - lce)
    new_ms, old_ms, read_ms = [], [], []
    roots = set()
    for r in range(rounds + 1):
        t0 = time.perf_counter()
        ev = ctx.constraint_evaluate(com, 0, prog, ext, lce)
        c_new, _ = ctx.constraint_commit_from_device_tables(p, [(ev, divs)])
        t1 = time.perf_counter()
        capi._check(L.wf_commitment_read_lde_strided(com._h, 0, 0, ce, stride, frame_buf.ctypes.data_as(C.c_void_p), C.byref(rw)))
        t2 = time.perf_counter()
        c_old, _ = ctx.constraint_commit_from_tables(p, [list(zip(host_cols, divs))])
        t3 = time.perf_counter()
        roots |= {c_new.root(), c_old.root()}
        ev.close(); c_new.close(); c_old.close()
        if r:  # round 0 warms tables and the buffer pool up
            new_ms.append((t1 - t0) * 1e3); old_ms.append((t3 - t1) * 1e3); read_ms.append((t2 - t1) * 1e3)
            print(f"round {r}: new {new_ms[-1]:8.2f} ms | old {old_ms[-1]:8.2f} ms (read_lde_strided {read_ms[-1]:.2f} + from_tables {old_ms[-1] - read_ms[-1]:.2f})", flush=True)
    assert len(roots) == 1, "the two routes disagree"
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"cfg {cfg} {name}: median new {med(new_ms):.2f} ms, old (lower bound) {med(old_ms):.2f} ms of which the read-back {med(read_ms):.2f} ms "
          f"({frame_buf.nbytes >> 20} MiB); ratio {med(old_ms) / med(new_ms):.2f}x; {ev.n_columns} columns of {host_cols[0].nbytes >> 20} MiB")
    # the kernel alone
    ctx.profile_enable(2)
    for _ in range(3):
        ctx.constraint_evaluate(com, 0, prog, ext, lce).close()
    ks = sorted(v for k, v in ctx.profile_read() if k == "constraint.evaluate")
    k_ms = ks[len(ks) // 2]
    types, cur, nxt = U.typing(g, ext)
    eb = 8 * w
    slots = len(cur) + len(nxt) + sum(ext if t == 2 else 1 for t in types if t) + any(s == U.X for _, _, a, b in g.instrs for s, _ in (a, b))
    best = (160 * 1024) // (64 * slots * eb) * 64
    group = next(gs for gs in (256, 128, 64) if (160 * 1024) // (gs * slots * eb) * gs == best)
    n_mul = 0
    live = [0] * g.n_regs
    for op, dst, a, b in g.instrs:
        e = [ext > 1 and (s == U.ECONST or (s == U.REG and live[i] == 2)) for s, i in (a, b)]
        live[dst] = 2 if any(e) else 1
        if op == U.MUL:
            n_mul += (3 if ext == 2 else 9) if all(e) else ext if any(e) else 1
    used = (len(cur) + len(nxt)) * eb * ce
    written = len(g.out_regs) * ext * eb * ce
    # (group size and slots restate csrc/cprog_plan.hpp -- tests/test_cprog_host.py holds the planner to the same rule; the library
    # has no call that reports its plan)
    line = (f"kernel {k_ms:.3f} ms: group {group} lanes, {slots} slots = {group * slots * eb} LDS bytes per group, {best // 64} waves per CU "
            f"by LDS; {len(g.instrs)} instructions, {n_mul} base products per step = {n_mul * ce / k_ms / 1e6:.1f} G products/s; "
            f"frame elements used {used >> 20} MiB + columns written {written >> 20} MiB = {(used + written) / k_ms / 1e9:.3f} TB/s")
    row_bytes = rw.value * eb
    if row_bytes <= 128 and len(cur) + len(nxt):
        # rows no longer than a cache line come in whole, whatever part of them is used: rows step << shift and their successors
        rows_touched = min(2, stride) * ce * row_bytes
        line += f" (whole rows touched: {rows_touched >> 20} MiB, {(rows_touched + written) / k_ms / 1e9:.3f} TB/s)"
    print(line)
    com.close()
    ctx.close()


def aux_route(rounds):
    """cfg 2's shape with an auxiliary segment: f64, 2^20 x 8 main columns, 4 auxiliary columns of the quadratic extension, ce
    blowup 4, the permutation argument on all four auxiliary columns (tests/cprog_aux_util.py: perm, n = 4)."""
    import ctypes as C
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import cprog_aux_util as A
    import cprog_util as U
    import edge_util as E
    field, logR, n_cols, n_aux, ext, logB, lce, n_cols_c = capi.F64, 20, 8, 4, 2, 3, 2, 2
    R, ce = 1 << logR, 1 << (logR + lce)
    ctx = capi.Context(0)
    rng = np.random.default_rng(2)
    com, _ = ctx.trace_commit_resident(capi.make_params(field, 1, logR, logB, n_cols, 1),
                                       [rng.integers(0, 2**62, size=R, dtype=np.uint64) for _ in range(n_cols)])
    aux, _ = ctx.trace_commit_resident(capi.make_params(field, ext, logR, logB, n_aux, 1),
                                       [rng.integers(0, 2**62, size=R * ext, dtype=np.uint64) for _ in range(n_aux)])
    g = A.perm(field, ext, [U.draw_e(rng, field, ext) for _ in range(n_aux)], n_aux)
    prog = U.to_capi(capi, g, field, ext)
    one = E.elements(field, [E.ONE[field]])
    gR = E.elements(field, [U.to_mem(field, pow(U.root_of_unity(field, logR), R - 1, U.P[field]))])
    divs = [(R, one, gR)] * n_aux + [(1, one, None)] * n_aux
    p = capi.make_params(field, ext, logR, logB, n_cols_c, 1)
    ev = ctx.constraint_evaluate_aux(com, 0, aux, 0, prog, ext, lce)
    host_cols = [ev.read(j) for j in range(ev.n_columns)]
    ev.close()
    L = capi.load()
    rw, arw = C.c_uint64(), C.c_uint64()
    L.wf_commitment_read_lde(com._h, 0, 0, 0, None, C.byref(rw))
    L.wf_commitment_read_lde(aux._h, 0, 0, 0, None, C.byref(arw))
    bufs = [np.zeros((ce, w.value), dtype=np.uint64) for w in (rw, arw)]   # touched: no page faults in the clock
    stride = 1 << (logB - lce)
    new_ms, old_ms, read_ms = [], [], []
    roots = set()
    for r in range(rounds + 1):
        t0 = time.perf_counter()
        ev = ctx.constraint_evaluate_aux(com, 0, aux, 0, prog, ext, lce)
        c_new, _ = ctx.constraint_commit_from_device_tables(p, [(ev, divs)])
        t1 = time.perf_counter()
        for h, buf, w in ((com, bufs[0], rw), (aux, bufs[1], arw)):
            capi._check(L.wf_commitment_read_lde_strided(h._h, 0, 0, ce, stride, buf.ctypes.data_as(C.c_void_p), C.byref(w)))
        t2 = time.perf_counter()
        c_old, _ = ctx.constraint_commit_from_tables(p, [list(zip(host_cols, divs))])
        t3 = time.perf_counter()
        roots |= {c_new.root(), c_old.root()}
        ev.close(); c_new.close(); c_old.close()
        if r:  # round 0 warms tables and the buffer pool up
            new_ms.append((t1 - t0) * 1e3); old_ms.append((t3 - t1) * 1e3); read_ms.append((t2 - t1) * 1e3)
            print(f"round {r}: new {new_ms[-1]:8.2f} ms | old {old_ms[-1]:8.2f} ms (read_lde_strided of both {read_ms[-1]:.2f} + from_tables {old_ms[-1] - read_ms[-1]:.2f})", flush=True)
    assert len(roots) == 1, "the two routes disagree"
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"aux perm x{n_aux}: median new {med(new_ms):.2f} ms, old (lower bound) {med(old_ms):.2f} ms of which the read-back {med(read_ms):.2f} ms "
          f"({sum(b.nbytes for b in bufs) >> 20} MiB); ratio {med(old_ms) / med(new_ms):.2f}x; {len(host_cols)} columns of {host_cols[0].nbytes >> 20} MiB")
    ctx.profile_enable(2)
    for _ in range(5):
        ctx.constraint_evaluate_aux(com, 0, aux, 0, prog, ext, lce).close()
    ks = sorted(v for k, v in ctx.profile_read() if k == "constraint.evaluate_aux")
    k_ms = ks[len(ks) // 2]
    types, cur, nxt, acur, anxt = A.typing(g, ext)
    used = (len(cur) + len(nxt) + (len(acur) + len(anxt)) * ext) * 8 * ce
    written = len(g.out_regs) * ext * 8 * ce
    # whole rows, per matrix the rows the program reads at all: step << shift and / or their successors (distinct: stride >= 2)
    rows = ce * 8 * (rw.value * (bool(cur) + bool(nxt)) + arw.value * (bool(acur) + bool(anxt)))
    print(f"kernel {ks[0]:.3f} / {k_ms:.3f} / {ks[-1]:.3f} ms (min / median / max of {len(ks)}): {len(g.instrs)} instructions; frame elements used "
          f"{used >> 20} MiB + columns written {written >> 20} MiB = {(used + written) / k_ms / 1e9:.3f} TB/s; whole rows touched {rows >> 20} MiB, "
          f"{(rows + written) / k_ms / 1e9:.3f} TB/s")
    com.close(); aux.close()
    ctx.close()


if len(sys.argv) > 1 and sys.argv[1] == "aux":
    aux_route(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "device":
    device_route(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 5, sys.argv[4] if len(sys.argv) > 4 else None)
    sys.exit(0)

logR = int(sys.argv[1]) if len(sys.argv) > 1 else 20
lce = int(sys.argv[2]) if len(sys.argv) > 2 else 1
ext, logB, n_cols = 2, 3, 2
R, ce = 1 << logR, 1 << (logR + lce)
ctx = capi.Context(0)
rng = np.random.default_rng(1)
r = lambda *shape: rng.integers(0, 2**62, size=shape, dtype=np.uint64)
one = np.array([0xFFFFFFFF], dtype=np.uint64)          # 1 in Montgomery form
p = capi.make_params(capi.F64, ext, logR, logB, n_cols, 1)
table = [(r(ce * ext), (R, one, r(1))), (r(ce * ext), (1, one, None))]
comb = r(ce * ext)
for rep in range(4):
    t0 = time.perf_counter()
    c1, _ = ctx.constraint_commit_from_tables(p, [table])
    t1 = time.perf_counter()
    c2, _ = ctx.constraint_commit_from_evaluations(p, [comb])
    t2 = time.perf_counter()
    c1.close(); c2.close()
    print(f"rep {rep}: from the table (2 columns of {ce * ext * 8 >> 20} MiB up) {(t1 - t0) * 1e3:.2f} ms; from the combined column (1 up) {(t2 - t1) * 1e3:.2f} ms", flush=True)
ctx.profile_enable(2)
c1, _ = ctx.constraint_commit_from_tables(p, [table])
acc = {}
for k, v in ctx.profile_read():
    acc.setdefault(k, []).append(round(v, 4))
print({k: v for k, v in acc.items() if k != "between_calls"})
