"""CPU: the constraint-program planner (csrc/cprog_plan.hpp) and the host-compiled step function of the interpreter
(csrc/cprog_dev.hpp) through tests/cpp/test_cprog_host.cpp, against tests/cprog_util.py -- the interpreter restated on Python
integers.  Built with plain g++ (WF_FIELD_LIMBS_ON_HOST: the device's formulation of the field arithmetic); the same program
runs a second time under -fsanitize=address,undefined as a stand-alone executable."""
import os
import subprocess

import numpy as np
import pytest

import cprog_util as U
import edge_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F128 = 1, 2
FIELDS = [(F64, 1), (F64, 2), (F64, 3), (F128, 1), (F128, 2)]
ERR_ARG, ERR_EXTENSION, ERR_BLOWUP = -19, -11, -13
LOG_R, LOG_B, LOG_CE_B, N_COLS = 4, 3, 2, 10  # ce = 64; 10 columns: rows of 16 with padding lanes


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_cprog_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_cprog_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cprog"))


def _words(field, values):
    if field == F64:
        return [str(v) for v in values]
    return [str(x) for v in values for x in (v & (2**64 - 1), v >> 64)]


def request(kind, field, ext, prog, *, n_cols=N_COLS, n_traces=1, trace_ext=1, log_r=LOG_R, log_b=LOG_B, has_lde=1, trace_index=0,
            log_ce_b=LOG_CE_B, nulls=0, counts=None, reserved=None, table_reserved=0, raw_consts=None, raw_table0=None, rows=None):
    """One request line.  counts: overrides of the structure's count fields; reserved: {instruction: (reserved0, reserved1)};
    raw_*: words sent as they are (values that are not field elements)."""
    counts = counts or {}
    t = [kind, field, trace_ext, n_cols, n_traces, log_r, log_b, has_lde, trace_index, ext, log_ce_b, 7 if field == F64 else 3, nulls]
    t += [counts.get("n_instrs", len(prog.instrs)), len(prog.instrs)]
    for i, (op, dst, a, b) in enumerate(prog.instrs):
        r0, r1 = (reserved or {}).get(i, (0, 0))
        t += [op, a[0], b[0], r0, dst, a[1], b[1], r1]
    t.append(counts.get("n_regs", prog.n_regs))
    t += [counts.get("n_consts", len(prog.consts)), len(prog.consts)] + (raw_consts or _words(field, prog.consts))
    flat = [c for e in prog.econsts for c in e]
    t += [counts.get("n_econsts", len(prog.econsts)), len(flat)] + _words(field, flat)
    t += [counts.get("n_tables", len(prog.tables)), len(prog.tables)]
    for k, (values, shift) in enumerate(prog.tables):
        log2_len = counts.get("log2_len", len(values).bit_length() - 1) if k == 0 else len(values).bit_length() - 1
        t += [log2_len, table_reserved if k == 0 else 0, shift, len(values)]
        t += raw_table0 if (k == 0 and raw_table0) else _words(field, values)
    t += [counts.get("n_out", len(prog.out_regs)), len(prog.out_regs)] + list(prog.out_regs)
    if rows is not None:
        t += [rows.shape[0], rows.shape[1]] + _words(field, rows.reshape(-1).tolist())
    return " ".join(str(x) for x in t)


def ask(exe, lines, env=None):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = []
    for l in res.stdout.splitlines():
        head, _, rest = l.partition(" ")
        rc = int(head)
        out.append((rc, rest if rc else [int(x) for x in rest.split()[1:]]))
    return out


def _lde(rng, field, n, n_cols):
    """(n, row_width) integers: the patterns of edge_util over the columns, zeros in the padding lanes"""
    rw = 8 * ((n_cols + 7) // 8)
    cols = [U.column_ints(field, c) for c in E.pattern_columns(rng, field, n_cols, n)]
    m = np.zeros((n, rw), dtype=object)
    for c, col in enumerate(cols):
        m[:, c] = col
    return m


_CASES = None


def _cases():
    """(request, expected flat list) for the five programs, every field and extension degree, ce = 64: computed once and shared
    by the plain and the sanitizer run."""
    global _CASES
    if _CASES is None:
        _CASES = []
        n, ce = 1 << (LOG_R + LOG_B), 1 << (LOG_R + LOG_CE_B)
        for field, ext in FIELDS:
            rng = np.random.default_rng(100 * field + ext)
            lde = _lde(rng, field, n, N_COLS)
            cur, nxt = U.frame_rows(lde, 1 << LOG_B, 1 << LOG_CE_B)
            xs = U.ce_points(field, ce, 7 if field == F64 else 3)
            for name in U.PROGRAMS:
                g = U.build(name, field, ext, rng, ce, 1 << LOG_CE_B, N_COLS)
                want = [v for col in U.evaluate(g, field, ext, cur, nxt, xs) for v in col]
                words = [x for v in want for x in ((v,) if field == F64 else (v & (2**64 - 1), v >> 64))]
                _CASES.append((f"{name} field {field} ext {ext}", request("RUN", field, ext, g, rows=lde), [len(g.out_regs), ce] + words))
    return _CASES


def _run_programs(exe, env=None):
    cases = _cases()
    got = ask(exe, [r for _, r, _ in cases], env)
    assert len(got) == len(cases)
    for (what, _, want), (rc, g) in zip(cases, got):
        assert rc == 0, f"{what}: {g}"
        assert g == want, what


def test_five_programs_match_the_python_reference(exe):
    _run_programs(exe)


def test_five_programs_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    san = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    _run_programs(san, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    # and the refusals: the planner must not read past what a refused program declares
    got = ask(san, [r for _, r, _, _ in refusals()], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert [rc for rc, _ in got] == [code for _, _, code, _ in refusals()]


def _small(field=F64, ext=2):
    """A valid program that uses every kind of pointer: 2 registers, a constant, an E constant, a table."""
    g = U.Prog(3)
    g.add(0, (U.CUR, 0), g.const(5))
    g.mul(0, (U.REG, 0), g.table([1, 2, 3, 4], shift=1))
    g.mul(1, (U.REG, 0), g.econst([3] * ext))
    g.out_regs = [1]
    return g


def _edit(g, i, **kw):
    """instruction i with fields replaced: op, dst, a, b"""
    op, dst, a, b = g.instrs[i]
    g.instrs[i] = (kw.get("op", op), kw.get("dst", dst), kw.get("a", a), kw.get("b", b))
    return g


def refusals():
    """(what, request, code, a word of the message) for every refusal of the header."""
    P64 = E.P64
    out = []

    def add(what, code, word, g=None, field=F64, ext=2, **kw):
        out.append((what, request("PLAN", field, ext, g or _small(field, ext if 1 <= ext <= 3 else 1), **kw), code, word))

    add("prog is null", ERR_ARG, "null", nulls=1)
    add("instrs is null", ERR_ARG, "null", nulls=2)
    add("out_regs is null", ERR_ARG, "null", nulls=4)
    add("consts is null", ERR_ARG, "null", nulls=8)
    add("econsts is null", ERR_ARG, "null", nulls=16)
    add("tables is null", ERR_ARG, "null", nulls=32)
    add("table values is null", ERR_ARG, "null", nulls=64)
    add("reserved0", ERR_ARG, "reserved", reserved={1: (1, 0)})
    add("reserved1", ERR_ARG, "reserved", reserved={0: (0, 7)})
    add("table reserved", ERR_ARG, "reserved", table_reserved=1)
    add("unknown op 0", ERR_ARG, "op", _edit(_small(), 0, op=0))
    add("unknown op 4", ERR_ARG, "op", _edit(_small(), 0, op=4))
    add("reserved source 7 (aux frame)", ERR_ARG, "source", _edit(_small(), 0, a=(7, 0)))
    add("unknown source 255", ERR_ARG, "source", _edit(_small(), 0, b=(255, 0)))
    add("n_instrs 0", ERR_ARG, "instructions", counts={"n_instrs": 0})
    add("n_instrs 4097", ERR_ARG, "instructions", counts={"n_instrs": 4097})
    add("n_regs 0", ERR_ARG, "registers", counts={"n_regs": 0})
    add("n_regs 65", ERR_ARG, "registers", counts={"n_regs": 65})
    add("n_out 0", ERR_ARG, "columns", counts={"n_out": 0})
    add("n_out 33", ERR_ARG, "columns", counts={"n_out": 33})
    add("dst out of range", ERR_ARG, "destination", _edit(_small(), 0, dst=3))
    add("register out of range", ERR_ARG, "register", _edit(_small(), 1, a=(U.REG, 3)))
    add("constant out of range", ERR_ARG, "constant", _edit(_small(), 0, b=(U.CONST, 1)))
    add("E constant out of range", ERR_ARG, "constant", _edit(_small(), 2, b=(U.ECONST, 1)))
    add("table out of range", ERR_ARG, "table", _edit(_small(), 1, b=(U.TABLE, 1)))
    add("column index == n_cols", ERR_ARG, "column", _edit(_small(), 0, a=(U.CUR, N_COLS)))
    add("NEXT column out of range", ERR_ARG, "column", _edit(_small(), 0, a=(U.NEXT, 200)))
    add("read before written", ERR_ARG, "before", _edit(_small(), 0, a=(U.REG, 1)))
    g = _small()
    g.add(0, (U.REG, 1), (U.REG, 1))  # register 0 is base, the sum of two E values is not
    add("second type", ERR_ARG, "second type", g)
    g = _small()
    g.out_regs = [2]
    add("out_regs never written", ERR_ARG, "never written", g)
    g = _small()
    g.out_regs = [3]
    add("out_regs out of range", ERR_ARG, "register", g)
    add("invalid constant (p)", ERR_ARG, "valid field element", raw_consts=[str(P64)])
    add("invalid constant (2^64 - 1)", ERR_ARG, "valid field element", raw_consts=[str(2**64 - 1)])
    add("invalid f128 constant (p)", ERR_ARG, "valid field element", field=F128, raw_consts=_words(F128, [E.P128]))
    add("invalid table value", ERR_ARG, "valid field element", raw_table0=["1", "2", str(P64 + 5), "4"])
    g = _small()
    g.tables[0] = (g.tables[0][0], 4)
    add("shift == len", ERR_ARG, "shift", g)
    g = _small()
    g.tables[0] = ([1] * 128, 0)
    add("len > ce", ERR_ARG, "exceed", g)
    add("trace_index == n_traces", ERR_ARG, "trace", n_traces=3, trace_index=3)
    for field, ext, fp in ((F64, 2, 64), (F64, 3, 64), (F128, 1, 32), (F128, 2, 32)):
        # one element over the footprint: E registers ext at a time, then base registers (64 registers of f64 with
        # ext_degree 1 are the limit itself: nothing to refuse there)
        g = U.Prog(64)
        n_e = 0 if ext == 1 else 4
        for r in range(n_e):
            g.mul(r, (U.CUR, 0), g.econst([1] * ext))
        for r in range(n_e, n_e + fp - n_e * ext + 1):
            g.add(r, (U.CUR, 0), (U.CUR, 1))
        g.out_regs = [0]
        add(f"footprint {fp + 1} field {field} ext {ext}", ERR_ARG, "base elements", g, field=field, ext=ext)
    # frame columns, x and registers share the 160 KiB of a compute unit: 320 f64 / 160 f128 slots for one wave
    add("frame that does not fit, f64 (322 slots)", ERR_ARG, "do not fit", U.wide_frame(F64, 129), ext=1, n_cols=130)
    add("frame that does not fit, f128 (162 slots)", ERR_ARG, "do not fit", U.wide_frame(F128, 65), field=F128, ext=1, n_cols=130)
    add("commitment of extension columns", ERR_ARG, "extension degree", trace_ext=2)
    add("commitment without rows", ERR_ARG, "no rows", has_lde=0)
    add("ext_degree 0", ERR_EXTENSION, "extension", ext=0)
    add("ext_degree 4", ERR_EXTENSION, "extension", ext=4)
    add("ext_degree 3 over f128", ERR_EXTENSION, "extension", field=F128, ext=3)
    add("log2_ce_blowup 0", ERR_BLOWUP, "blowup", log_ce_b=0)
    add("log2_ce_blowup > log2_blowup", ERR_BLOWUP, "blowup", log_ce_b=LOG_B + 1)
    return out


_REFUSALS = refusals()


@pytest.mark.parametrize("what,req,code,word", _REFUSALS, ids=[r[0] for r in _REFUSALS])
def test_refusal(exe, what, req, code, word):
    ((rc, msg),) = ask(exe, [req])
    assert rc == code, msg
    assert word in msg, msg


def test_the_footprint_limit_itself_is_accepted(exe):
    reqs = []
    for field, ext in FIELDS:
        fp = U.MAX_FOOTPRINT[field]
        g = U.Prog(64)
        n_e = 0 if ext == 1 else 4
        for r in range(n_e):
            g.mul(r, (U.CUR, 0), g.econst([1] * ext))
        for r in range(n_e, n_e + fp - n_e * ext):
            g.add(r, (U.CUR, 0), (U.CUR, 1))
        g.out_regs = [0]
        reqs.append(request("PLAN", field, ext, g))
    for (field, ext), (rc, ans) in zip(FIELDS, ask(exe, reqs)):
        assert rc == 0, ans
        group, lds, n_slots = ans[:3]
        assert n_slots == 2 + U.MAX_FOOTPRINT[field]          # two frame columns and the registers
        assert lds == group * n_slots * (8 if field == F64 else 16) <= 160 * 1024 and group in (64, 128, 256)


def test_a_frame_that_just_fits_takes_all_of_a_compute_unit(exe):
    reqs = [request("PLAN", F64, 1, U.wide_frame(F64, 128), n_cols=130), request("PLAN", F128, 1, U.wide_frame(F128, 64), n_cols=130)]
    for n_slots, (rc, ans) in zip((320, 160), ask(exe, reqs)):
        assert rc == 0, ans
        assert ans[:3] == [64, 160 * 1024, n_slots]


def _random_program(rng, field, ext, n_cols, ce):
    """A random VALID program: random sizes, registers typed by their first write, a few never written."""
    n_regs = int(rng.integers(1, 20))
    g = U.Prog(n_regs)
    for _ in range(int(rng.integers(1, 4))):
        g.const(int(rng.integers(0, 1000)))
    for _ in range(int(rng.integers(1, 3))):
        g.econst([int(rng.integers(0, 1000)) for _ in range(ext)])
    g.table([1, 2], 1)
    g.table(list(range(8)), int(rng.integers(0, 8)))
    types = {}
    for _ in range(int(rng.integers(1, 40))):
        dst = int(rng.integers(0, n_regs))
        ops = []
        for _ in range(2):
            k = int(rng.integers(0, 7))
            regs = sorted(types)
            if k == U.REG and not regs:
                k = U.CUR
            idx = {U.REG: lambda: regs[int(rng.integers(0, len(regs)))], U.CUR: lambda: int(rng.integers(0, n_cols)),
                   U.NEXT: lambda: int(rng.integers(0, n_cols)), U.CONST: lambda: int(rng.integers(0, len(g.consts))),
                   U.ECONST: lambda: int(rng.integers(0, len(g.econsts))), U.TABLE: lambda: int(rng.integers(0, 2)),
                   U.X: lambda: int(rng.integers(0, 9))}[k]()
            ops.append((k, idx))
        is_e = ext > 1 and any((k == U.ECONST) or (k == U.REG and types[i] == 2) for k, i in ops)
        t = 2 if is_e else 1
        if types.get(dst, t) != t:
            continue
        types[dst] = t
        g.op(int(rng.integers(1, 4)), dst, ops[0], ops[1])
    if not g.instrs:
        g.add(0, (U.CUR, 0), (U.X, 0))
        types[0] = 1
    written = sorted(types)
    g.out_regs = [written[int(rng.integers(0, len(written)))] for _ in range(int(rng.integers(1, 5)))]
    return g


def test_planner_on_1000_random_valid_programs(exe):
    """Slots are disjoint, the types are the reference typing, the set of frame columns is exactly what the program reads, and
    the op of every instruction is split by the operand types."""
    rng = np.random.default_rng(2024)
    progs, reqs = [], []
    for k in range(1000):
        field, ext = FIELDS[k % len(FIELDS)]
        n_cols = int(rng.integers(1, 12))
        g = _random_program(rng, field, ext, n_cols, 64)
        progs.append((field, ext, n_cols, g))
        reqs.append(request("PLAN", field, ext, g, n_cols=n_cols))
    answers = ask(exe, reqs)
    assert len(answers) == 1000
    for (field, ext, n_cols, g), (rc, a) in zip(progs, answers):
        assert rc == 0, a
        group, lds, n_slots, x_slot, reg_base, n_frame = a[:6]
        frame = a[6:6 + n_frame]
        k = 6 + n_frame
        n_regs = a[k]
        regs = [(a[k + 1 + 2 * r], a[k + 2 + 2 * r]) for r in range(n_regs)]
        k += 1 + 2 * n_regs
        codes = a[k + 1:k + 1 + a[k]]
        types, cur, nxt = U.typing(g, ext)
        assert [t for t, _ in regs] == types
        assert sorted(frame) == sorted(list(cur) + [c | (1 << 16) for c in nxt])
        taken = list(range(n_frame))                      # frame entry i lives in slot i
        uses_x = any(s == U.X for _, _, a_, b_ in g.instrs for s, _ in (a_, b_))
        assert (x_slot != 0xFFFFFFFF) == uses_x
        if uses_x:
            taken.append(x_slot)
        for t, slot in regs:
            if t:
                assert slot >= reg_base
                taken += list(range(slot, slot + (ext if t == 2 else 1)))
        assert len(set(taken)) == len(taken) == n_slots and max(taken) == n_slots - 1
        eb = 8 if field == F64 else 16
        assert group in (64, 128, 256) and lds == group * n_slots * eb <= 160 * 1024
        # the largest group that loses no lane of a compute unit to granularity
        best = (160 * 1024) // (64 * n_slots * eb) * 64
        assert (160 * 1024) // (group * n_slots * eb) * group == best
        assert all((160 * 1024) // (gg * n_slots * eb) * gg < best for gg in (128, 256) if gg > group)
        assert len(codes) == len(g.instrs)
        live = [0] * g.n_regs
        for code, (op, dst, a_, b_) in zip(codes, g.instrs):
            e = [ext > 1 and (s == U.ECONST or (s == U.REG and live[i] == 2)) for s, i in (a_, b_)]
            assert code == (op - 1) * 4 + (1 if e[0] else 0) + (2 if e[1] else 0)
            live[dst] = 2 if any(e) else 1
