"""CPU: the constraint-program planner with an auxiliary segment (cprog_plan_aux, csrc/cprog_plan.hpp) and the host-compiled
step function (csrc/cprog_dev.hpp) on a main and an auxiliary matrix, through tests/cpp/test_cprog_aux_host.cpp, against
tests/cprog_aux_util.py -- the interpreter with both auxiliary sources restated on Python integers.  Built with plain g++; the
same program runs a second time under -fsanitize=address,undefined as a stand-alone executable (nothing is preloaded)."""
import os
import subprocess

import numpy as np
import pytest

import cprog_aux_util as A
import cprog_util as U
import edge_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F128 = 1, 2
FIELDS = [(F64, 1), (F64, 2), (F64, 3), (F128, 1), (F128, 2)]
ERR_ARG, ERR_EXTENSION, ERR_BLOWUP = -19, -11, -13
LOG_R, LOG_B, LOG_CE_B, N_COLS, N_AUX = 4, 3, 2, 10, 5  # ce = 64; 10 main columns: rows of 16; 5 aux columns of E
SLOTS = {F64: 320, F128: 160}                            # base elements of one wave's lanes in 160 KiB


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_cprog_aux_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_cprog_aux_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cprog_aux"))


def _words(field, values):
    if field == F64:
        return [str(v) for v in values]
    return [str(x) for v in values for x in (v & (2**64 - 1), v >> 64)]


def request(kind, field, ext, prog, *, n_cols=N_COLS, n_traces=1, trace_ext=1, log_r=LOG_R, log_b=LOG_B, has_lde=1, trace_index=0,
            log_ce_b=LOG_CE_B, aux=None, null_prog=0, rows=None, aux_rows=None):
    """One request line.  aux: overrides of the auxiliary shape (field, trace_ext, n_cols, n_traces, log_r, log_b, has_lde, index);
    by default the main commitment's parameters with ext_degree = ext and N_AUX columns."""
    a = dict(field=field, trace_ext=ext, n_cols=N_AUX, n_traces=1, log_r=log_r, log_b=log_b, has_lde=1, index=0)
    a.update(aux or {})
    t = [kind, field, trace_ext, n_cols, n_traces, log_r, log_b, has_lde, trace_index, ext, log_ce_b, 7 if field == F64 else 3]
    t += [a["field"], a["trace_ext"], a["n_cols"], a["n_traces"], a["log_r"], a["log_b"], a["has_lde"], a["index"], null_prog]
    t.append(len(prog.instrs))
    for op, dst, x, y in prog.instrs:
        t += [op, x[0], y[0], dst, x[1], y[1]]
    t.append(prog.n_regs)
    t += [len(prog.consts)] + _words(field, prog.consts)
    flat = [c for e in prog.econsts for c in e]
    t += [len(flat)] + _words(field, flat)
    t.append(len(prog.tables))
    for values, shift in prog.tables:
        t += [len(values).bit_length() - 1, shift, len(values)] + _words(field, values)
    t += [len(prog.out_regs)] + list(prog.out_regs)
    for m in (rows, aux_rows):
        if m is not None:
            t += [m.shape[0], m.shape[1]] + _words(field, m.reshape(-1).tolist())
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


def _matrix(rng, field, n, n_cols, ext=1):
    """(n, row width) integers: the patterns of edge_util over the columns, coordinates of an element side by side.  The row is
    exactly n_cols * ext wide for the auxiliary matrix (no padding lane hides a read past the last column) and padded to a
    multiple of 8 for the main one, as a resident commitment stores it."""
    rw = n_cols * ext if ext > 1 else 8 * ((n_cols + 7) // 8)
    m = np.zeros((n, rw), dtype=object)
    for c, col in enumerate(E.pattern_columns(rng, field, n_cols, n, ext=ext)):
        ints = U.column_ints(field, col)
        for w in range(ext):
            m[:, c * ext + w] = ints[w::ext]
    return m


_CASES = None


def _cases():
    """(what, request, expected flat list) for the four auxiliary programs and the five main-only ones, every field and extension
    degree, ce = 64: computed once and shared by the plain and the sanitizer run."""
    global _CASES
    if _CASES is None:
        _CASES = []
        n, ce = 1 << (LOG_R + LOG_B), 1 << (LOG_R + LOG_CE_B)
        for field, ext in FIELDS:
            rng = np.random.default_rng(1000 * field + ext)
            lde = _matrix(rng, field, n, N_COLS)
            aux = _matrix(rng, field, n, N_AUX, ext) if ext > 1 else _matrix(rng, field, n, N_AUX)[:, :N_AUX]
            cur, nxt = U.frame_rows(lde, 1 << LOG_B, 1 << LOG_CE_B)
            acur, anxt = U.frame_rows(aux, 1 << LOG_B, 1 << LOG_CE_B)
            xs = U.ce_points(field, ce, 7 if field == F64 else 3)
            progs = [(name, A.build(name, field, ext, rng, ce, 1 << LOG_CE_B, N_COLS, N_AUX)) for name in A.AUX_PROGRAMS]
            progs += [(name, U.build(name, field, ext, rng, ce, 1 << LOG_CE_B, N_COLS)) for name in U.PROGRAMS]
            for name, g in progs:
                want = [v for col in A.evaluate(g, field, ext, cur, nxt, acur, anxt, xs) for v in col]
                if name in U.PROGRAMS:
                    assert want == [v for col in U.evaluate(g, field, ext, cur, nxt, xs) for v in col]
                words = [x for v in want for x in ((v,) if field == F64 else (v & (2**64 - 1), v >> 64))]
                _CASES.append((f"{name} field {field} ext {ext}", request("RUN", field, ext, g, rows=lde, aux_rows=aux),
                               [len(g.out_regs), ce] + words))
    return _CASES


def _run_programs(exe, env=None):
    cases = _cases()
    got = ask(exe, [r for _, r, _ in cases], env)
    assert len(got) == len(cases)
    for (what, _, want), (rc, g) in zip(cases, got):
        assert rc == 0, f"{what}: {g}"
        assert g == want, what


def test_the_stress_program_covers_every_source_kind_on_both_sides(exe):
    """.. and the planner finds every auxiliary column in both rows of its frame"""
    progs = [A.aux_stress(field, ext, np.random.default_rng(3), 64, N_COLS, N_AUX) for field, ext in FIELDS]
    answers = ask(exe, [request("PLAN", field, ext, g) for (field, ext), g in zip(FIELDS, progs)])
    for (field, ext), g, (rc, ans) in zip(FIELDS, progs, answers):
        ka, kb, acur, anxt = A.stress_coverage(g)
        assert ka == kb == set(range(9)) and acur == anxt == set(range(N_AUX)) and len(g.instrs) == 300
        types = A.typing(g, ext)[0]
        assert sum(ext if t == 2 else 1 for t in types if t) == U.MAX_FOOTPRINT[field]
        assert rc == 0, ans
        n_frame = ans[5]
        aux_base, n_aux_frame = ans[6 + n_frame], ans[7 + n_frame]
        assert aux_base == n_frame and ans[8 + n_frame:8 + n_frame + n_aux_frame] == list(range(N_AUX)) + [c | (1 << 16) for c in range(N_AUX)]


def test_aux_programs_match_the_python_reference(exe):
    _run_programs(exe)


def test_aux_programs_and_refusals_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    san = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    _run_programs(san, env=env)
    got = ask(san, [r for _, r, _, _ in _REFUSALS], env=env)
    assert [rc for rc, _ in got] == [code for _, _, code, _ in _REFUSALS]


def _small(ext=2):
    """A valid program that reads both frames, a constant, an E constant and a table."""
    g = U.Prog(3)
    g.add(0, (U.CUR, 0), g.const(5))
    g.mul(0, (U.REG, 0), g.table([1, 2, 3, 4], shift=1))
    g.mul(1, (A.AUX_CUR, 0), g.econst([3] * ext))
    g.add(1, (U.REG, 1), (A.AUX_NEXT, N_AUX - 1))
    g.mul(1, (U.REG, 1), (U.REG, 0))
    g.out_regs = [1]
    return g


def _edit(g, i, **kw):
    op, dst, a, b = g.instrs[i]
    g.instrs[i] = (kw.get("op", op), kw.get("dst", dst), kw.get("a", a), kw.get("b", b))
    return g


def refusals():
    """(what, request, code, a word of the message): every refusal that the auxiliary call adds, and those of the main call that
    it must keep with their codes."""
    out = []

    def add(what, code, word, g=None, field=F64, ext=2, kind="PLAN", **kw):
        e = ext if 1 <= ext <= 3 else 1
        out.append((what, request(kind, field, ext, g or _small(e), **kw), code, word))

    add("prog is null", ERR_ARG, "null", null_prog=1)
    add("aux field differs", ERR_ARG, "shape", aux=dict(field=F128))
    add("aux log2_trace_len differs", ERR_ARG, "shape", aux=dict(log_r=LOG_R + 1))
    add("aux log2_blowup differs", ERR_ARG, "shape", aux=dict(log_b=LOG_B - 1))
    add("aux ext_degree 1 for a program in degree 2", ERR_ARG, "extension degree", aux=dict(trace_ext=1))
    add("aux ext_degree 3 for a program in degree 2", ERR_ARG, "extension degree", aux=dict(trace_ext=3))
    add("aux ext_degree 2 for a program in degree 1", ERR_ARG, "extension degree", _small(1), ext=1, aux=dict(trace_ext=2))
    add("aux commitment without rows", ERR_ARG, "no rows", aux=dict(has_lde=0))
    add("aux_index == n_traces", ERR_ARG, "trace", aux=dict(n_traces=3, index=3))
    add("AUX_CUR column == n_cols", ERR_ARG, "column", _edit(_small(), 2, a=(A.AUX_CUR, N_AUX)))
    add("AUX_NEXT column out of range", ERR_ARG, "column", _edit(_small(), 3, b=(A.AUX_NEXT, 200)))
    add("aux column in range of the main columns only", ERR_ARG, "column", _edit(_small(), 2, a=(A.AUX_CUR, N_COLS - 1)))
    add("source 9", ERR_ARG, "source", _edit(_small(), 0, a=(9, 0)))
    add("source 255", ERR_ARG, "source", _edit(_small(), 0, b=(255, 0)))
    add("source 7 through cprog_plan", ERR_ARG, "source", _edit(_small(), 3, b=(U.CONST, 0)), kind="OLD")
    add("source 8 through cprog_plan", ERR_ARG, "source", _edit(_small(), 2, a=(U.CUR, 0)), kind="OLD")
    g = _small()
    g.add(0, (U.REG, 0), (A.AUX_CUR, 0))  # register 0 is base; a sum with an auxiliary element is of type E
    add("an aux operand makes the op an E op: second type", ERR_ARG, "second type", g)
    # the frame budget: 320 f64 / 160 f128 base elements for main frame, aux frame at ext each, x and registers
    for field, ext, n_main, n_aux, use_x in _JUST_FITS:
        assert A.wide_aux_slots(field, ext, n_main, n_aux, use_x) == SLOTS[field]
        add(f"one aux column more than fits, field {field} ext {ext}", ERR_ARG, "do not fit",
            A.wide_aux_frame(field, ext, n_main, n_aux + 1, use_x), field=field, ext=ext, n_cols=n_main, aux=dict(n_cols=n_aux + 1))
    # the main call's refusals, with their codes
    add("main commitment of extension columns", ERR_ARG, "extension degree", trace_ext=2)
    add("main commitment without rows", ERR_ARG, "no rows", has_lde=0)
    add("trace_index == n_traces", ERR_ARG, "trace", n_traces=3, trace_index=3)
    add("main column out of range", ERR_ARG, "column", _edit(_small(), 0, a=(U.CUR, N_COLS)))
    add("ext_degree 0", ERR_EXTENSION, "extension", ext=0, aux=dict(trace_ext=0))
    add("ext_degree 4", ERR_EXTENSION, "extension", ext=4, aux=dict(trace_ext=4))
    add("ext_degree 3 over f128", ERR_EXTENSION, "extension", _small(3), field=F128, ext=3)
    add("log2_ce_blowup 0", ERR_BLOWUP, "blowup", log_ce_b=0)
    add("log2_ce_blowup > log2_blowup", ERR_BLOWUP, "blowup", log_ce_b=LOG_B + 1)
    for field, ext in ((F64, 2), (F128, 2)):
        fp = U.MAX_FOOTPRINT[field]
        g = U.Prog(64)
        for r in range(fp // ext):
            g.mul(r, (A.AUX_CUR, 0), (A.AUX_NEXT, 1))
        g.add(fp // ext, (U.CUR, 0), (U.CUR, 1))
        g.out_regs = [0]
        add(f"footprint {fp + 1} field {field} ext {ext}", ERR_ARG, "base elements", g, field=field, ext=ext)
    return out


#             field, ext, main columns, aux columns, x: exactly 320 (f64) / 160 (f128) slots
_JUST_FITS = [(F64, 1, 100, 28, False), (F64, 2, 8, 60, False), (F64, 3, 113, 5, True), (F128, 1, 34, 30, False), (F128, 2, 2, 31, False)]
_REFUSALS = refusals()


@pytest.mark.parametrize("what,req,code,word", _REFUSALS, ids=[r[0] for r in _REFUSALS])
def test_refusal(exe, what, req, code, word):
    ((rc, msg),) = ask(exe, [req])
    assert rc == code, msg
    assert word in msg, msg


def test_an_aux_frame_that_just_fits_takes_all_of_a_compute_unit(exe):
    reqs = [request("PLAN", field, ext, A.wide_aux_frame(field, ext, n_main, n_aux, use_x), n_cols=n_main, aux=dict(n_cols=n_aux))
            for field, ext, n_main, n_aux, use_x in _JUST_FITS]
    for (field, ext, n_main, n_aux, use_x), (rc, ans) in zip(_JUST_FITS, ask(exe, reqs)):
        assert rc == 0, ans
        assert ans[:3] == [64, 160 * 1024, SLOTS[field]]
        n_frame = ans[5]
        assert n_frame == 2 * n_main and ans[6 + n_frame] == 2 * n_main and ans[7 + n_frame] == 2 * n_aux


def test_the_footprint_limit_with_an_aux_frame_is_accepted(exe):
    reqs = []
    for field, ext in FIELDS:
        fp = U.MAX_FOOTPRINT[field]
        g = U.Prog(64)
        n_e = 0 if ext == 1 else 4
        for r in range(n_e):
            g.mul(r, (A.AUX_CUR, 0), (A.AUX_NEXT, 1))
        for r in range(n_e, n_e + fp - n_e * ext):
            g.add(r, (U.CUR, 0), (U.CUR, 1) if ext > 1 else (A.AUX_NEXT, 1))
        g.out_regs = [0]
        reqs.append(request("PLAN", field, ext, g))
    for (field, ext), (rc, ans) in zip(FIELDS, ask(exe, reqs)):
        assert rc == 0, ans
        group, lds, n_slots = ans[:3]
        n_aux_read = 2 if ext > 1 else 1
        n_main_read = 2 if ext > 1 else 1
        assert n_slots == n_main_read + n_aux_read * ext + U.MAX_FOOTPRINT[field]
        assert lds == group * n_slots * (8 if field == F64 else 16) <= 160 * 1024 and group in (64, 128, 256)


def _random_program(rng, field, ext, n_cols, n_aux):
    """A random VALID program with auxiliary sources: registers typed by their first write, a few never written."""
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
            k = int(rng.integers(0, 9))
            regs = sorted(types)
            if k == U.REG and not regs:
                k = A.AUX_CUR
            idx = {U.REG: lambda: regs[int(rng.integers(0, len(regs)))], U.CUR: lambda: int(rng.integers(0, n_cols)),
                   U.NEXT: lambda: int(rng.integers(0, n_cols)), U.CONST: lambda: int(rng.integers(0, len(g.consts))),
                   U.ECONST: lambda: int(rng.integers(0, len(g.econsts))), U.TABLE: lambda: int(rng.integers(0, 2)),
                   U.X: lambda: int(rng.integers(0, 9)), A.AUX_CUR: lambda: int(rng.integers(0, n_aux)),
                   A.AUX_NEXT: lambda: int(rng.integers(0, n_aux))}[k]()
            ops.append((k, idx))
        is_e = ext > 1 and any((k in (U.ECONST, A.AUX_CUR, A.AUX_NEXT)) or (k == U.REG and types[i] == 2) for k, i in ops)
        t = 2 if is_e else 1
        if types.get(dst, t) != t:
            continue
        types[dst] = t
        g.op(int(rng.integers(1, 4)), dst, ops[0], ops[1])
    if not g.instrs:
        g.add(0, (A.AUX_NEXT, 0), (U.X, 0))
        types[0] = 2 if ext > 1 else 1
    written = sorted(types)
    g.out_regs = [written[int(rng.integers(0, len(written)))] for _ in range(int(rng.integers(1, 5)))]
    return g


def test_planner_on_1000_random_valid_programs_with_aux_sources(exe):
    """Slots are disjoint and an E entry takes ext of them, the two frame sets are exactly what the program reads (ascending, CUR
    before NEXT), the types are the reference typing, every operand resolves to its slot, the group is the largest that loses no
    lane -- and with the auxiliary sources stripped the plan is cprog_plan's, field for field."""
    rng = np.random.default_rng(2025)
    progs, reqs, same = [], [], []
    for k in range(1000):
        field, ext = FIELDS[k % len(FIELDS)]
        n_cols, n_aux = int(rng.integers(1, 12)), int(rng.integers(1, 7))
        g = _random_program(rng, field, ext, n_cols, n_aux)
        progs.append((field, ext, n_cols, n_aux, g))
        reqs.append(request("PLAN", field, ext, g, n_cols=n_cols, aux=dict(n_cols=n_aux)))
        same.append(request("SAME", field, ext, A.strip_aux(g), n_cols=n_cols, aux=dict(n_cols=n_aux)))
    answers = ask(exe, reqs)
    assert len(answers) == 1000
    assert [a for a in ask(exe, same)] == [(0, [1])] * 1000
    n_with_aux = 0
    for (field, ext, n_cols, n_aux, g), (rc, a) in zip(progs, answers):
        assert rc == 0, a
        group, lds, n_slots, x_slot, reg_base, n_frame = a[:6]
        frame = a[6:6 + n_frame]
        k = 6 + n_frame
        aux_base, n_aux_frame = a[k], a[k + 1]
        aux_frame = a[k + 2:k + 2 + n_aux_frame]
        k += 2 + n_aux_frame
        n_regs = a[k]
        regs = [(a[k + 1 + 2 * r], a[k + 2 + 2 * r]) for r in range(n_regs)]
        k += 1 + 2 * n_regs
        n_instrs = a[k]
        kin = [a[k + 1 + 6 * i:k + 7 + 6 * i] for i in range(n_instrs)]
        types, cur, nxt, acur, anxt = A.typing(g, ext)
        n_with_aux += bool(acur or anxt)
        assert [t for t, _ in regs] == types
        assert frame == sorted(cur) + [c | (1 << 16) for c in sorted(nxt)]
        assert aux_frame == sorted(acur) + [c | (1 << 16) for c in sorted(anxt)]
        assert aux_base == n_frame
        taken = list(range(n_frame)) + list(range(aux_base, aux_base + n_aux_frame * ext))
        uses_x = any(s == U.X for _, _, a_, b_ in g.instrs for s, _ in (a_, b_))
        assert (x_slot != 0xFFFFFFFF) == uses_x
        if uses_x:
            assert x_slot == aux_base + n_aux_frame * ext
            taken.append(x_slot)
        for t, slot in regs:
            if t:
                assert slot >= reg_base
                taken += list(range(slot, slot + (ext if t == 2 else 1)))
        assert len(set(taken)) == len(taken) == n_slots and max(taken) == n_slots - 1
        eb = 8 if field == F64 else 16
        assert group in (64, 128, 256) and lds == group * n_slots * eb <= 160 * 1024
        best = (160 * 1024) // (64 * n_slots * eb) * 64
        assert (160 * 1024) // (group * n_slots * eb) * group == best
        assert all((160 * 1024) // (gg * n_slots * eb) * gg < best for gg in (128, 256) if gg > group)
        assert n_instrs == len(g.instrs)
        live = [0] * g.n_regs
        slot_of = {(U.CUR, c): i for i, c in enumerate(sorted(cur))}
        slot_of.update({(U.NEXT, c): len(cur) + i for i, c in enumerate(sorted(nxt))})
        slot_of.update({(A.AUX_CUR, c): aux_base + i * ext for i, c in enumerate(sorted(acur))})
        slot_of.update({(A.AUX_NEXT, c): aux_base + (len(acur) + i) * ext for i, c in enumerate(sorted(anxt))})
        for (code, a_kind, a_v, b_kind, b_v, dst), (op, d, a_, b_) in zip(kin, g.instrs):
            e = [ext > 1 and (s in (U.ECONST, A.AUX_CUR, A.AUX_NEXT) or (s == U.REG and live[i] == 2)) for s, i in (a_, b_)]
            assert code == (op - 1) * 4 + (1 if e[0] else 0) + (2 if e[1] else 0)
            assert dst == regs[d][1]
            for (s, i), kind, v in ((a_, a_kind, a_v), (b_, b_kind, b_v)):
                if (s, i) in slot_of:
                    assert (kind, v) == (0, slot_of[(s, i)])      # CPK_LDS
                elif s == U.REG:
                    assert (kind, v) == (0, regs[i][1])
                elif s == U.X:
                    assert (kind, v) == (0, x_slot)
            live[d] = 2 if any(e) else 1
    assert n_with_aux > 900
