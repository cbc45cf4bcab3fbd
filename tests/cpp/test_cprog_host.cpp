// CPU driver of the constraint-program planner (csrc/cprog_plan.hpp) and of the host-compiled step function
// (csrc/cprog_dev.hpp) for tests/test_cprog_host.py.  Request-driven: whitespace-separated tokens on stdin, one answer line per
// request on stdout.  Plain g++ (the headers are __host__ __device__ / HIP-free); WF_FIELD_LIMBS_ON_HOST makes the field
// arithmetic the device's 32-bit-limb formulation.
//
//   request  := kind shape nulls program [rows]
//   kind     := PLAN | RUN
//   shape    := field trace_ext n_cols n_traces log2_trace_len log2_blowup has_lde trace_index ext log2_ce_blowup offset
//   nulls    := bit mask: 1 prog, 2 instrs, 4 out_regs, 8 consts, 16 econsts, 32 tables, 64 values of table 0
//   program  := n_instrs count {op a_src b_src reserved0 dst a b reserved1}*count   n_regs
//               n_consts count {element}*count   n_econsts count {element}*count
//               n_tables count {log2_len reserved shift n_values {element}*n_values}*count   n_out count {reg}*count
//               (n_x: the value of the structure's field; count: how many entries -- for econsts base elements -- follow)
//   element  := one (f64) or two (f128: lo hi) unsigned 64-bit words
//   rows     := n_rows row_width {element}*(n_rows * row_width)      (RUN: the LDE matrix)
//   answer   := PLAN: rc | group_size lds_bytes n_slots x_slot reg_base n_frame {frame}* n_regs {type slot}* n_instrs {code}*
//               RUN:  rc | n_out ce {element}*(n_out * ce * ext)
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

template <class F, int WE>
static void run(const wf_cprog &prog, const CpPlan &pl, const CpShape &sh, uint32_t trace_index, const std::vector<uint64_t> &rows,
                uint64_t n_rows, uint64_t row_width, unsigned __int128 offset) {
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
    const T *lde = (const T *)rows.data();
    const uint32_t log_ce = sh.log2_trace_len + sh.log2_blowup - pl.lde_shift;
    const T g = f_root_of_unity<F>(log_ce);
    T x = F::from_u128_canonical(offset);
    const uint64_t n = (uint64_t)1 << (sh.log2_trace_len + sh.log2_blowup);
    if (n_rows != n || row_width < sh.n_cols) {
        fprintf(stderr, "matrix of %llu x %llu for %llu rows of %u columns\n", (unsigned long long)n_rows, (unsigned long long)row_width,
                (unsigned long long)n, sh.n_cols);
        exit(3);
    }
    (void)trace_index;
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
            s.set_slot((uint32_t)i, lde[((pl.frame[i] >> 16) ? rn : rc) * row_width + (pl.frame[i] & 0xFFFF)]);
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

int main() {
    std::string kind;
    while (std::cin >> kind) {
        const bool is_run = kind == "RUN";
        if (!is_run && kind != "PLAN") {
            fprintf(stderr, "unknown request %s\n", kind.c_str());
            return 3;
        }
        CpShape sh;
        sh.field = (uint32_t)tok();
        sh.trace_ext = (uint32_t)tok();
        sh.n_cols = (uint32_t)tok();
        sh.n_traces = (uint32_t)tok();
        sh.log2_trace_len = (uint32_t)tok();
        sh.log2_blowup = (uint32_t)tok();
        sh.has_lde = tok() != 0;
        const uint32_t trace_index = (uint32_t)tok(), ext = (uint32_t)tok(), log2_ce_blowup = (uint32_t)tok();
        const uint64_t offset = tok(), nulls = tok();
        const size_t w = sh.field == WF_FIELD_F128 ? 2 : 1;
        wf_cprog prog;
        memset(&prog, 0, sizeof(prog));
        prog.n_instrs = (uint32_t)tok();
        std::vector<wf_cprog_instr> instrs(tok());
        for (auto &in : instrs) {
            in.op = (uint8_t)tok();
            in.a_src = (uint8_t)tok();
            in.b_src = (uint8_t)tok();
            in.reserved0 = (uint8_t)tok();
            in.dst = (uint16_t)tok();
            in.a = (uint16_t)tok();
            in.b = (uint16_t)tok();
            in.reserved1 = (uint16_t)tok();
        }
        prog.n_regs = (uint32_t)tok();
        prog.n_consts = (uint32_t)tok();
        std::vector<uint64_t> consts(tok() * w);
        for (auto &v : consts) v = tok();
        prog.n_econsts = (uint32_t)tok();
        std::vector<uint64_t> econsts(tok() * w);
        for (auto &v : econsts) v = tok();
        prog.n_tables = (uint32_t)tok();
        std::vector<wf_cprog_table> tables(tok());
        std::vector<std::vector<uint64_t>> tvals(tables.size());
        for (size_t t = 0; t < tables.size(); t++) {
            tables[t].log2_len = (uint32_t)tok();
            tables[t].reserved = (uint32_t)tok();
            tables[t].shift = tok();
            tvals[t].resize(tok() * w);
            for (auto &v : tvals[t]) v = tok();
            tables[t].values = (t == 0 && (nulls & 64)) ? nullptr : tvals[t].data();
        }
        prog.n_out = (uint32_t)tok();
        std::vector<uint16_t> outs(tok());
        for (auto &v : outs) v = (uint16_t)tok();
        prog.instrs = (nulls & 2) ? nullptr : instrs.data();
        prog.out_regs = (nulls & 4) ? nullptr : outs.data();
        prog.consts = (nulls & 8) ? nullptr : consts.data();
        prog.econsts = (nulls & 16) ? nullptr : econsts.data();
        prog.tables = (nulls & 32) ? nullptr : tables.data();
        uint64_t n_rows = 0, row_width = 0;
        std::vector<uint64_t> rows;
        if (is_run) {
            n_rows = tok();
            row_width = tok();
            rows.resize(n_rows * row_width * w);
            for (auto &v : rows) v = tok();
        }
        CpPlan pl;
        const int rc = cprog_plan((nulls & 1) ? nullptr : &prog, sh, trace_index, ext, log2_ce_blowup, pl);
        if (rc) {
            printf("%d # %s\n", rc, pl.msg);
            continue;
        }
        if (!is_run) {
            printf("0 | %u %u %u %u %u %zu", pl.group_size, pl.lds_bytes, pl.n_slots, pl.x_slot, pl.reg_base, pl.frame.size());
            for (uint32_t f : pl.frame) printf(" %u", f);
            printf(" %zu", pl.reg_type.size());
            for (size_t r = 0; r < pl.reg_type.size(); r++) printf(" %u %u", pl.reg_type[r], pl.reg_slot[r]);
            printf(" %zu", pl.instrs.size());
            for (const CpInstr &in : pl.instrs) printf(" %u", in.code());
            printf("\n");
            continue;
        }
        if (sh.field == WF_FIELD_F64) {
            if (ext == 1) run<F64, 1>(prog, pl, sh, trace_index, rows, n_rows, row_width, offset);
            else if (ext == 2) run<F64, 2>(prog, pl, sh, trace_index, rows, n_rows, row_width, offset);
            else run<F64, 3>(prog, pl, sh, trace_index, rows, n_rows, row_width, offset);
        } else {
            if (ext == 1) run<F128, 1>(prog, pl, sh, trace_index, rows, n_rows, row_width, offset);
            else run<F128, 2>(prog, pl, sh, trace_index, rows, n_rows, row_width, offset);
        }
    }
    return 0;
}
