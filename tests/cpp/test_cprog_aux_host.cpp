// CPU driver of the constraint-program planner with an auxiliary segment (cprog_plan_aux, csrc/cprog_plan.hpp) and of the
// host-compiled step function (csrc/cprog_dev.hpp) for tests/test_cprog_aux_host.py.  Request-driven like test_cprog_host.cpp:
// whitespace-separated tokens on stdin, one answer line per request on stdout.  Plain g++; WF_FIELD_LIMBS_ON_HOST makes the
// field arithmetic the device's 32-bit-limb formulation.
//
//   request  := kind shape aux nulls program [rows aux_rows]
//   kind     := PLAN | RUN | OLD | SAME
//               PLAN / RUN: cprog_plan_aux;  OLD: cprog_plan (no auxiliary shape, whatever `aux` says);
//               SAME: the program through cprog_plan_aux and through cprog_plan -- are the two plans equal field for field
//   shape    := field trace_ext n_cols n_traces log2_trace_len log2_blowup has_lde trace_index ext log2_ce_blowup offset
//   aux      := field trace_ext n_cols n_traces log2_trace_len log2_blowup has_lde aux_index
//   nulls    := bit mask: 1 prog
//   program  := n_instrs {op a_src b_src dst a b}*n_instrs   n_regs   n_consts {element}*   n_econsts*ext {element}*
//               n_tables {log2_len shift n_values {element}*n_values}*   n_out {reg}*
//   element  := one (f64) or two (f128: lo hi) unsigned 64-bit words
//   rows     := n_rows row_width {element}*(n_rows * row_width)      (RUN: the main matrix, then the auxiliary matrix)
//   answer   := PLAN / OLD: rc | group_size lds_bytes n_slots x_slot reg_base n_frame {frame}* aux_base n_aux {aux_frame}*
//                                n_regs {type slot}* n_instrs {code a_kind a b_kind b dst}*
//               RUN:  rc | n_out ce {element}*(n_out * ce * ext)
//               SAME: rc | 0 or 1
//               refused: rc # message
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <string>
#include <vector>

#define WF_FIELD_LIMBS_ON_HOST 1
#include "../../starkpack-winterfell_amd/csrc/cprog_dev.hpp"

using namespace wf;

static uint64_t tok() {
    std::string s;
    if (!(std::cin >> s)) {
        fprintf(stderr, "request ends early\n");
        exit(3);
    }
    return strtoull(s.c_str(), nullptr, 10);
}

template <class F>
struct HostLane {
    typedef typename F::T T;
    std::vector<T> slots;
    const T *consts;
    const CpTable *tables;
    const T *table_values;
    uint64_t step;
    T slot(uint32_t s) const { return slots.at(s); }
    void set_slot(uint32_t s, T v) { slots.at(s) = v; }
    T constant(uint32_t off) const { return consts[off]; }
    T table(uint32_t t) const {
        const CpTable d = tables[t];
        return table_values[d.offset + (((uint32_t)step - d.shift) & d.mask)];
    }
};

static void put(uint64_t v) { printf(" %llu", (unsigned long long)v); }
static void put(const U128 &v) { printf(" %llu %llu", (unsigned long long)v.lo, (unsigned long long)v.hi); }

struct Matrix {
    std::vector<uint64_t> words;
    uint64_t n_rows = 0, row_width = 0;
};

static Matrix read_matrix(size_t w) {
    Matrix m;
    m.n_rows = tok();
    m.row_width = tok();
    m.words.resize(m.n_rows * m.row_width * w);
    for (auto &v : m.words) v = tok();
    return m;
}

template <class F, int WE>
static void run(const wf_cprog &prog, const CpPlan &pl, const CpShape &sh, const CpShape &sa, const Matrix &mm, const Matrix &am,
                unsigned __int128 offset) {
    typedef typename F::T T;
    const size_t eb = sizeof(T);
    // the buffers as constraint_eval.hip fills them
    std::vector<T> consts(pl.n_const_elems + 1), tvals(pl.n_table_elems + 1);
    size_t off = 0;
    for (uint32_t src : pl.const_src) {
        const bool is_e = src >> 31;
        const size_t idx = src & 0x7FFFFFFFu, nb = is_e ? WE * eb : eb;
        memcpy((char *)consts.data() + off, (const char *)(is_e ? prog.econsts : prog.consts) + idx * nb, nb);
        off += nb;
    }
    for (size_t t = 0; t < pl.tables.size(); t++)
        memcpy(&tvals[pl.tables[t].offset], prog.tables[pl.table_src[t]].values, ((size_t)pl.tables[t].mask + 1) * eb);
    const uint64_t n = (uint64_t)1 << (sh.log2_trace_len + sh.log2_blowup);
    if (mm.n_rows != n || mm.row_width < sh.n_cols || am.n_rows != n || am.row_width < (uint64_t)sa.n_cols * WE) {
        fprintf(stderr, "matrices of %llu x %llu and %llu x %llu for %llu rows\n", (unsigned long long)mm.n_rows,
                (unsigned long long)mm.row_width, (unsigned long long)am.n_rows, (unsigned long long)am.row_width, (unsigned long long)n);
        exit(3);
    }
    // own copies of exactly the declared size: a read past a row's end is the sanitizer's to find
    std::vector<T> lde(mm.n_rows * mm.row_width), aux(am.n_rows * am.row_width);
    memcpy(lde.data(), mm.words.data(), lde.size() * eb);
    memcpy(aux.data(), am.words.data(), aux.size() * eb);
    const uint32_t log_ce = sh.log2_trace_len + sh.log2_blowup - pl.lde_shift;
    const T g = f_root_of_unity<F>(log_ce);
    T x = F::from_u128_canonical(offset);
    std::vector<T> out((size_t)prog.n_out * pl.ce * WE);
    HostLane<F> s;
    s.consts = consts.data();
    s.tables = pl.tables.data();
    s.table_values = tvals.data();
    for (uint64_t step = 0; step < pl.ce; step++) {
        s.slots.assign(pl.n_slots, F::zero());
        s.step = step;
        const uint64_t rc = step << pl.lde_shift, rn = (rc + ((uint64_t)1 << sh.log2_blowup)) & (n - 1);
        for (size_t i = 0; i < pl.frame.size(); i++)
            s.set_slot((uint32_t)i, lde.at(((pl.frame[i] >> 16) ? rn : rc) * mm.row_width + (pl.frame[i] & 0xFFFF)));
        for (size_t i = 0; i < pl.aux_frame.size(); i++)
            for (int w = 0; w < WE; w++)
                s.set_slot(pl.aux_base + (uint32_t)i * WE + w,
                           aux.at(((pl.aux_frame[i] >> 16) ? rn : rc) * am.row_width + (size_t)(pl.aux_frame[i] & 0xFFFF) * WE + w));
        if (pl.x_slot != CP_NO_SLOT) s.set_slot(pl.x_slot, x);
        for (const CpInstr &in : pl.instrs) cprog_step<F, WE>(in, s);
        for (uint32_t j = 0; j < prog.n_out; j++)
            for (int w = 0; w < WE; w++)
                out[((size_t)j * pl.ce + step) * WE + w] = (w == 0 || pl.out_is_ext[j]) ? s.slot(pl.out_slot[j] + w) : F::zero();
        x = F::mul(x, g);
    }
    printf("0 | %u %llu", prog.n_out, (unsigned long long)pl.ce);
    for (const T &v : out) put(v);
    printf("\n");
}

static bool same_instrs(const std::vector<CpInstr> &a, const std::vector<CpInstr> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].op != b[i].op || a[i].dst != b[i].dst || a[i].a != b[i].a || a[i].b != b[i].b) return false;
    return true;
}
static bool same_tables(const std::vector<CpTable> &a, const std::vector<CpTable> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].offset != b[i].offset || a[i].mask != b[i].mask || a[i].shift != b[i].shift || a[i].pad != b[i].pad) return false;
    return true;
}
// every member but msg, aux_frame and aux_base (which cprog_plan leaves empty / at the end of the frame)
static bool same_plan(const CpPlan &p, const CpPlan &q) {
    return p.field == q.field && p.ext == q.ext && p.ce == q.ce && p.lde_shift == q.lde_shift && same_instrs(p.instrs, q.instrs) &&
           p.reg_type == q.reg_type && p.reg_slot == q.reg_slot && p.frame == q.frame && p.x_slot == q.x_slot && p.reg_base == q.reg_base &&
           p.reg_footprint == q.reg_footprint && p.n_slots == q.n_slots && p.const_src == q.const_src && p.n_const_elems == q.n_const_elems &&
           p.table_src == q.table_src && same_tables(p.tables, q.tables) && p.n_table_elems == q.n_table_elems && p.out_slot == q.out_slot &&
           p.out_is_ext == q.out_is_ext && p.group_size == q.group_size && p.lds_bytes == q.lds_bytes && p.n_mul == q.n_mul &&
           p.aux_frame.empty() && q.aux_frame.empty() && p.aux_base == p.frame.size() && q.aux_base == q.frame.size();
}

static void read_shape(CpShape &sh) {
    sh.field = (uint32_t)tok();
    sh.trace_ext = (uint32_t)tok();
    sh.n_cols = (uint32_t)tok();
    sh.n_traces = (uint32_t)tok();
    sh.log2_trace_len = (uint32_t)tok();
    sh.log2_blowup = (uint32_t)tok();
    sh.has_lde = tok() != 0;
}

int main() {
    std::string kind;
    while (std::cin >> kind) {
        const bool is_run = kind == "RUN", is_old = kind == "OLD", is_same = kind == "SAME";
        if (!is_run && !is_old && !is_same && kind != "PLAN") {
            fprintf(stderr, "unknown request %s\n", kind.c_str());
            return 3;
        }
        CpShape sh, sa;
        read_shape(sh);
        const uint32_t trace_index = (uint32_t)tok(), ext = (uint32_t)tok(), log2_ce_blowup = (uint32_t)tok();
        const uint64_t offset = tok();
        read_shape(sa);
        const uint32_t aux_index = (uint32_t)tok();
        const uint64_t nulls = tok();
        const size_t w = sh.field == WF_FIELD_F128 ? 2 : 1;
        wf_cprog prog;
        memset(&prog, 0, sizeof(prog));
        prog.n_instrs = (uint32_t)tok();
        std::vector<wf_cprog_instr> instrs(prog.n_instrs);
        for (auto &in : instrs) {
            memset(&in, 0, sizeof(in));
            in.op = (uint8_t)tok();
            in.a_src = (uint8_t)tok();
            in.b_src = (uint8_t)tok();
            in.dst = (uint16_t)tok();
            in.a = (uint16_t)tok();
            in.b = (uint16_t)tok();
        }
        prog.n_regs = (uint32_t)tok();
        prog.n_consts = (uint32_t)tok();
        std::vector<uint64_t> consts(prog.n_consts * w);
        for (auto &v : consts) v = tok();
        const size_t n_econst_elems = tok();
        const uint32_t e = ext >= 1 && ext <= 3 ? ext : 1;
        prog.n_econsts = (uint32_t)(n_econst_elems / e);
        std::vector<uint64_t> econsts(n_econst_elems * w);
        for (auto &v : econsts) v = tok();
        prog.n_tables = (uint32_t)tok();
        std::vector<wf_cprog_table> tables(prog.n_tables);
        std::vector<std::vector<uint64_t>> tvals(tables.size());
        for (size_t t = 0; t < tables.size(); t++) {
            tables[t].log2_len = (uint32_t)tok();
            tables[t].reserved = 0;
            tables[t].shift = tok();
            tvals[t].resize(tok() * w);
            for (auto &v : tvals[t]) v = tok();
            tables[t].values = tvals[t].data();
        }
        prog.n_out = (uint32_t)tok();
        std::vector<uint16_t> outs(prog.n_out);
        for (auto &v : outs) v = (uint16_t)tok();
        prog.instrs = instrs.data();
        prog.out_regs = outs.data();
        prog.consts = consts.data();
        prog.econsts = econsts.data();
        prog.tables = tables.data();
        Matrix mm, am;
        if (is_run) {
            mm = read_matrix(w);
            am = read_matrix(w);
        }
        CpPlan pl;
        const wf_cprog *pp = (nulls & 1) ? nullptr : &prog;
        const int rc = is_old ? cprog_plan(pp, sh, trace_index, ext, log2_ce_blowup, pl)
                              : cprog_plan_aux(pp, sh, &sa, trace_index, aux_index, ext, log2_ce_blowup, pl);
        if (rc) {
            printf("%d # %s\n", rc, pl.msg);
            continue;
        }
        if (is_same) {
            CpPlan old;
            const int rc2 = cprog_plan(pp, sh, trace_index, ext, log2_ce_blowup, old);
            if (rc2) {
                printf("%d # %s\n", rc2, old.msg);
                continue;
            }
            printf("0 | %d\n", same_plan(pl, old) ? 1 : 0);
            continue;
        }
        if (!is_run) {
            printf("0 | %u %u %u %u %u %zu", pl.group_size, pl.lds_bytes, pl.n_slots, pl.x_slot, pl.reg_base, pl.frame.size());
            for (uint32_t f : pl.frame) printf(" %u", f);
            printf(" %u %zu", pl.aux_base, pl.aux_frame.size());
            for (uint32_t f : pl.aux_frame) printf(" %u", f);
            printf(" %zu", pl.reg_type.size());
            for (size_t r = 0; r < pl.reg_type.size(); r++) printf(" %u %u", pl.reg_type[r], pl.reg_slot[r]);
            printf(" %zu", pl.instrs.size());
            for (const CpInstr &in : pl.instrs) printf(" %u %u %u %u %u %u", in.code(), in.a_kind(), in.a, in.b_kind(), in.b, in.dst);
            printf("\n");
            continue;
        }
        if (sh.field == WF_FIELD_F64) {
            if (ext == 1) run<F64, 1>(prog, pl, sh, sa, mm, am, offset);
            else if (ext == 2) run<F64, 2>(prog, pl, sh, sa, mm, am, offset);
            else run<F64, 3>(prog, pl, sh, sa, mm, am, offset);
        } else {
            if (ext == 1) run<F128, 1>(prog, pl, sh, sa, mm, am, offset);
            else run<F128, 2>(prog, pl, sh, sa, mm, am, offset);
        }
    }
    return 0;
}
