// Host planning of a constraint program (wf_constraint_evaluate, constraint_eval.hip) as pure host code: no HIP in this header,
// so tests/cpp/test_cprog_host.cpp runs it under plain g++.
//
// A constraint program (wf_cprog, include/wf_lde.h) is a straight-line program of field additions, subtractions and products
// over the two rows of the evaluation frame, constants, periodic-style tables and the domain point; one interpreter kernel
// (cprog_kernels.hpp) runs it for every step of the constraint evaluation domain.  The planner
//   - refuses whatever the header lists as refused (cprog_plan returns the status, CpPlan::msg says why),
//   - infers the type of every register (base field or E; fixed by the first write),
//   - collects the frame columns the program reads (the kernel loads only those),
//   - lays the lane's state out in LDS slots of one base element: [frame columns][aux frame columns][x][registers], an E
//     register and an aux frame column WE slots,
//   - rewrites the program into the kernel's form: the op split by operand types (BB / EB / BE / EE), REG / CUR / NEXT / X
//     resolved to slots, CONST / ECONST to offsets into one constant buffer that holds only what is referenced, TABLE to an
//     entry of the table descriptors (again only the referenced ones),
//   - chooses the work-group size from the LDS footprint.
// cprog_plan_aux is the planner of wf_constraint_evaluate_aux: with the shape of an auxiliary commitment it accepts the sources
// AUX_CUR / AUX_NEXT (elements of E of the auxiliary segment's frame, trace_lde.rs:100-108); cprog_plan is the same function
// without one, where those kinds stay unknown sources.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/wf_lde.h"

namespace wf {

// source kinds of the kernel's instruction form
enum : uint8_t { CPK_LDS = 0, CPK_CONST = 1, CPK_TABLE = 2 };
// code = (op - 1) * 4 + (a is E) + 2 * (b is E):  BB = 0, EB = 1, BE = 2, EE = 3 within an op
enum : uint8_t { CPT_BB = 0, CPT_EB = 1, CPT_BE = 2, CPT_EE = 3 };

struct alignas(16) CpInstr {  // four whole words: the scalar unit loads words, not bytes -- one 16-byte wave-uniform load
    uint32_t op;   // code | a_kind << 8 | b_kind << 16
    uint32_t dst;  // slot
    uint32_t a, b; // slot (CPK_LDS), element offset into the constant buffer, or table entry
    constexpr uint32_t code() const { return op & 0xFFu; }  // (constexpr: callable from host and device code alike)
    constexpr uint32_t a_kind() const { return (op >> 8) & 0xFFu; }
    constexpr uint32_t b_kind() const { return (op >> 16) & 0xFFu; }
};
struct CpTable {
    uint32_t offset;  // first value in the table buffer (elements)
    uint32_t mask;    // length - 1
    uint32_t shift;   // value at `step` is values[(step - shift) & mask]
    uint32_t pad;
};

// what the planner needs to know of the commitment the program runs on
struct CpShape {
    uint32_t field;           // enum wf_field
    uint32_t trace_ext;       // wf_params::ext_degree of the commitment (must be 1: main segment)
    uint32_t n_cols, n_traces;
    uint32_t log2_trace_len, log2_blowup;
    bool has_lde;
};

constexpr uint32_t CP_MAX_INSTRS = 4096, CP_MAX_REGS = 64, CP_MAX_OUT = 32;
constexpr uint32_t CP_LDS_BYTES = 160 * 1024;  // per CU (gfx950)
constexpr uint32_t CP_NO_SLOT = 0xFFFFFFFFu;

struct CpPlan {
    char msg[200];
    uint32_t field = 0, ext = 0;
    uint64_t ce = 0;
    uint32_t lde_shift = 0;                // lde_step = step << lde_shift
    std::vector<CpInstr> instrs;
    std::vector<uint8_t> reg_type;         // per caller register: 0 never written, 1 base, 2 E
    std::vector<uint32_t> reg_slot;        // first slot of a written register
    std::vector<uint32_t> frame;           // column | (NEXT ? 1 << 16 : 0), ascending; entry i lives in slot i
    std::vector<uint32_t> aux_frame;       // the same of the auxiliary segment (columns of E); entry i lives in slots aux_base + i * ext ..
    uint32_t aux_base = 0;
    uint32_t x_slot = CP_NO_SLOT;
    uint32_t reg_base = 0, reg_footprint = 0, n_slots = 0;
    std::vector<uint32_t> const_src;       // the constant buffer: index | (ECONST ? 1 << 31 : 0), an ECONST takes ext elements
    uint32_t n_const_elems = 0;
    std::vector<uint32_t> table_src;       // caller's table index of descriptor i
    std::vector<CpTable> tables;
    uint64_t n_table_elems = 0;
    std::vector<uint32_t> out_slot;        // first slot of evaluation column j
    std::vector<uint8_t> out_is_ext;
    uint32_t group_size = 0, lds_bytes = 0;
    uint32_t n_mul = 0;                    // base-field products of one step (BB 1, EB / BE ext, EE 3 or 9): for rate reports
};

inline int cp_fail(CpPlan &pl, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
inline int cp_fail(CpPlan &pl, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(pl.msg, sizeof(pl.msg), fmt, ap);
    va_end(ap);
    return code;
}

// a base-field element in memory representation: f64 a Montgomery residue < p, f128 a canonical integer < p
inline bool cp_valid_elem(uint32_t field, const void *p) {
    if (field == WF_FIELD_F64) {
        uint64_t v;
        memcpy(&v, p, 8);
        return v < 0xFFFFFFFF00000001ull;
    }
    uint64_t w[2];
    memcpy(w, p, 16);
    return w[1] != 0xFFFFFFFFFFFFFFFFull || w[0] < 0xFFFFD30000000001ull;
}

// Work-group size: LDS holds 160 KiB / (bytes per lane) lanes of a CU whatever the group size, so the largest group that
// loses none of them to granularity is taken (fewer groups to dispatch, and the uniform instruction stream is fetched once per
// wave either way).  0: not even one wave fits.
inline uint32_t cp_group_size(uint32_t bytes_per_lane) {
    const uint32_t best = CP_LDS_BYTES / (64 * bytes_per_lane) * 64;  // lanes of a CU with one-wave groups
    if (best == 0) return 0;
    for (uint32_t g = 256; g > 64; g >>= 1)
        if (CP_LDS_BYTES / (g * bytes_per_lane) * g == best) return g;
    return 64;
}

// sh_aux == nullptr: main segment only (wf_constraint_evaluate)
inline int cprog_plan_aux(const wf_cprog *prog, const CpShape &sh, const CpShape *sh_aux, uint32_t trace_index, uint32_t aux_index,
                          uint32_t ext_degree, uint32_t log2_ce_blowup, CpPlan &pl) {
    pl.msg[0] = 0;
    if (!prog) return cp_fail(pl, WF_ERR_ARG, "prog is null");
    if (sh.field != WF_FIELD_F64 && sh.field != WF_FIELD_F128) return cp_fail(pl, WF_ERR_FIELD, "unknown field id %u", sh.field);
    if (sh.trace_ext != 1)
        return cp_fail(pl, WF_ERR_ARG, "the commitment holds columns of extension degree %u: only main trace segments (degree 1) are evaluated",
                       sh.trace_ext);
    if (!sh.has_lde) return cp_fail(pl, WF_ERR_ARG, "this commitment holds no rows");
    if (trace_index >= sh.n_traces) return cp_fail(pl, WF_ERR_ARG, "trace %u of %u", trace_index, sh.n_traces);
    if (ext_degree < 1 || ext_degree > 3 || (sh.field == WF_FIELD_F128 && ext_degree == 3))
        return cp_fail(pl, WF_ERR_EXTENSION, "unsupported extension degree %u for field %u", ext_degree, sh.field);
    if (log2_ce_blowup == 0 || log2_ce_blowup > sh.log2_blowup)
        return cp_fail(pl, WF_ERR_BLOWUP, "constraint evaluation blowup 2^%u is not in [2, 2^%u]", log2_ce_blowup, sh.log2_blowup);
    if (sh_aux) {
        if (sh_aux->field != sh.field || sh_aux->log2_trace_len != sh.log2_trace_len || sh_aux->log2_blowup != sh.log2_blowup)
            return cp_fail(pl, WF_ERR_ARG, "the auxiliary commitment (field %u, 2^%u rows, blowup 2^%u) is not of the main commitment's shape (field %u, 2^%u rows, blowup 2^%u)",
                           sh_aux->field, sh_aux->log2_trace_len, sh_aux->log2_blowup, sh.field, sh.log2_trace_len, sh.log2_blowup);
        if (sh_aux->trace_ext != ext_degree)
            return cp_fail(pl, WF_ERR_ARG, "the auxiliary commitment holds columns of extension degree %u, the program runs in degree %u",
                           sh_aux->trace_ext, ext_degree);
        if (!sh_aux->has_lde) return cp_fail(pl, WF_ERR_ARG, "the auxiliary commitment holds no rows");
        if (aux_index >= sh_aux->n_traces) return cp_fail(pl, WF_ERR_ARG, "auxiliary trace %u of %u", aux_index, sh_aux->n_traces);
    }
    const uint32_t eb = sh.field == WF_FIELD_F64 ? 8 : 16, WE = ext_degree;
    const uint64_t ce = (uint64_t)1 << (sh.log2_trace_len + log2_ce_blowup);
    pl.field = sh.field;
    pl.ext = WE;
    pl.ce = ce;
    pl.lde_shift = sh.log2_blowup - log2_ce_blowup;

    if (!prog->instrs) return cp_fail(pl, WF_ERR_ARG, "instrs is null");
    if (!prog->out_regs) return cp_fail(pl, WF_ERR_ARG, "out_regs is null");
    if (prog->n_instrs < 1 || prog->n_instrs > CP_MAX_INSTRS)
        return cp_fail(pl, WF_ERR_ARG, "%u instructions (1 to %u)", prog->n_instrs, CP_MAX_INSTRS);
    if (prog->n_regs < 1 || prog->n_regs > CP_MAX_REGS) return cp_fail(pl, WF_ERR_ARG, "%u registers (1 to %u)", prog->n_regs, CP_MAX_REGS);
    if (prog->n_out < 1 || prog->n_out > CP_MAX_OUT) return cp_fail(pl, WF_ERR_ARG, "%u evaluation columns (1 to %u)", prog->n_out, CP_MAX_OUT);
    if (prog->n_consts && !prog->consts) return cp_fail(pl, WF_ERR_ARG, "consts is null");
    if (prog->n_econsts && !prog->econsts) return cp_fail(pl, WF_ERR_ARG, "econsts is null");
    if (prog->n_tables && !prog->tables) return cp_fail(pl, WF_ERR_ARG, "tables is null");
    for (uint32_t k = 0; k < prog->n_consts; k++)
        if (!cp_valid_elem(sh.field, (const char *)prog->consts + (size_t)k * eb))
            return cp_fail(pl, WF_ERR_ARG, "constant %u is not a valid field element", k);
    for (uint64_t k = 0; k < (uint64_t)prog->n_econsts * WE; k++)
        if (!cp_valid_elem(sh.field, (const char *)prog->econsts + (size_t)k * eb))
            return cp_fail(pl, WF_ERR_ARG, "extension constant %u is not a valid field element", (uint32_t)(k / WE));
    for (uint32_t t = 0; t < prog->n_tables; t++) {
        const wf_cprog_table &tb = prog->tables[t];
        if (!tb.values) return cp_fail(pl, WF_ERR_ARG, "table %u: values is null", t);
        if (tb.reserved) return cp_fail(pl, WF_ERR_ARG, "table %u: reserved field is not zero", t);
        if (tb.log2_len > 63 || ((uint64_t)1 << tb.log2_len) > ce)
            return cp_fail(pl, WF_ERR_ARG, "table %u: 2^%u values exceed the %llu steps of the domain", t, tb.log2_len, (unsigned long long)ce);
        const uint64_t len = (uint64_t)1 << tb.log2_len;
        if (tb.shift >= len) return cp_fail(pl, WF_ERR_ARG, "table %u: shift %llu of %llu values", t, (unsigned long long)tb.shift, (unsigned long long)len);
        for (uint64_t k = 0; k < len; k++)
            if (!cp_valid_elem(sh.field, (const char *)tb.values + (size_t)k * eb))
                return cp_fail(pl, WF_ERR_ARG, "table %u: value %llu is not a valid field element", t, (unsigned long long)k);
    }

    // ---- pass 1: validate, infer the types, collect what is read
    const uint32_t NI = prog->n_instrs;
    pl.reg_type.assign(prog->n_regs, 0);
    std::vector<uint8_t> cur_used(sh.n_cols, 0), next_used(sh.n_cols, 0);
    const uint32_t n_aux_cols = sh_aux ? sh_aux->n_cols : 0;
    std::vector<uint8_t> aux_cur_used(n_aux_cols, 0), aux_next_used(n_aux_cols, 0);
    std::vector<uint8_t> typing(NI);
    bool x_used = false;
    for (uint32_t i = 0; i < NI; i++) {
        const wf_cprog_instr &in = prog->instrs[i];
        if (in.reserved0 || in.reserved1) return cp_fail(pl, WF_ERR_ARG, "instruction %u: reserved field is not zero", i);
        if (in.op < WF_CP_ADD || in.op > WF_CP_MUL) return cp_fail(pl, WF_ERR_ARG, "instruction %u: unknown op %u", i, in.op);
        uint8_t ty[2];
        for (int o = 0; o < 2; o++) {
            const uint32_t src = o ? in.b_src : in.a_src, idx = o ? in.b : in.a;
            ty[o] = 1;
            switch (src) {
                case WF_CP_REG:
                    if (idx >= prog->n_regs) return cp_fail(pl, WF_ERR_ARG, "instruction %u: register %u of %u", i, idx, prog->n_regs);
                    if (!pl.reg_type[idx]) return cp_fail(pl, WF_ERR_ARG, "instruction %u: register %u is read before it is written", i, idx);
                    ty[o] = pl.reg_type[idx];
                    break;
                case WF_CP_CUR:
                case WF_CP_NEXT:
                    if (idx >= sh.n_cols) return cp_fail(pl, WF_ERR_ARG, "instruction %u: column %u of %u", i, idx, sh.n_cols);
                    (src == WF_CP_CUR ? cur_used : next_used)[idx] = 1;
                    break;
                case WF_CP_CONST:
                    if (idx >= prog->n_consts) return cp_fail(pl, WF_ERR_ARG, "instruction %u: constant %u of %u", i, idx, prog->n_consts);
                    break;
                case WF_CP_ECONST:
                    if (idx >= prog->n_econsts) return cp_fail(pl, WF_ERR_ARG, "instruction %u: extension constant %u of %u", i, idx, prog->n_econsts);
                    if (WE > 1) ty[o] = 2;  // with ext_degree 1 the two types coincide
                    break;
                case WF_CP_TABLE:
                    if (idx >= prog->n_tables) return cp_fail(pl, WF_ERR_ARG, "instruction %u: table %u of %u", i, idx, prog->n_tables);
                    break;
                case WF_CP_X:
                    x_used = true;
                    break;
                case WF_CP_AUX_CUR:
                case WF_CP_AUX_NEXT:
                    if (!sh_aux) return cp_fail(pl, WF_ERR_ARG, "instruction %u: unknown operand source %u", i, src);
                    if (idx >= n_aux_cols) return cp_fail(pl, WF_ERR_ARG, "instruction %u: auxiliary column %u of %u", i, idx, n_aux_cols);
                    (src == WF_CP_AUX_CUR ? aux_cur_used : aux_next_used)[idx] = 1;
                    if (WE > 1) ty[o] = 2;
                    break;
                default:
                    return cp_fail(pl, WF_ERR_ARG, "instruction %u: unknown operand source %u", i, src);
            }
        }
        if (in.dst >= prog->n_regs) return cp_fail(pl, WF_ERR_ARG, "instruction %u: destination register %u of %u", i, in.dst, prog->n_regs);
        const uint8_t rt = (ty[0] == 2 || ty[1] == 2) ? 2 : 1;
        if (pl.reg_type[in.dst] && pl.reg_type[in.dst] != rt)
            return cp_fail(pl, WF_ERR_ARG, "instruction %u: register %u is written with a second type", i, in.dst);
        if (!pl.reg_type[in.dst]) {
            pl.reg_type[in.dst] = rt;
            pl.reg_footprint += rt == 2 ? WE : 1;
        }
        typing[i] = (uint8_t)((ty[0] == 2 ? 1 : 0) | (ty[1] == 2 ? 2 : 0));
        pl.n_mul += in.op != WF_CP_MUL ? 0 : typing[i] == CPT_BB ? 1 : typing[i] == CPT_EE ? (WE == 2 ? 3 : 9) : WE;
    }
    for (uint32_t j = 0; j < prog->n_out; j++) {
        const uint32_t r = prog->out_regs[j];
        if (r >= prog->n_regs) return cp_fail(pl, WF_ERR_ARG, "evaluation column %u: register %u of %u", j, r, prog->n_regs);
        if (!pl.reg_type[r]) return cp_fail(pl, WF_ERR_ARG, "evaluation column %u: register %u is never written", j, r);
    }
    const uint32_t max_fp = sh.field == WF_FIELD_F64 ? 64 : 32;
    if (pl.reg_footprint > max_fp)
        return cp_fail(pl, WF_ERR_ARG, "the registers take %u base elements (at most %u)", pl.reg_footprint, max_fp);

    // ---- slots: [frame columns][aux frame columns, WE slots each][x][registers in register order]
    std::vector<uint32_t> cur_slot(sh.n_cols, CP_NO_SLOT), next_slot(sh.n_cols, CP_NO_SLOT);
    pl.frame.clear();
    for (uint32_t c = 0; c < sh.n_cols; c++)
        if (cur_used[c]) {
            cur_slot[c] = (uint32_t)pl.frame.size();
            pl.frame.push_back(c);
        }
    for (uint32_t c = 0; c < sh.n_cols; c++)
        if (next_used[c]) {
            next_slot[c] = (uint32_t)pl.frame.size();
            pl.frame.push_back(c | (1u << 16));
        }
    uint32_t slot = (uint32_t)pl.frame.size();
    std::vector<uint32_t> aux_cur_slot(n_aux_cols, CP_NO_SLOT), aux_next_slot(n_aux_cols, CP_NO_SLOT);
    pl.aux_frame.clear();
    pl.aux_base = slot;
    for (uint32_t c = 0; c < n_aux_cols; c++)
        if (aux_cur_used[c]) {
            aux_cur_slot[c] = pl.aux_base + (uint32_t)pl.aux_frame.size() * WE;
            pl.aux_frame.push_back(c);
        }
    for (uint32_t c = 0; c < n_aux_cols; c++)
        if (aux_next_used[c]) {
            aux_next_slot[c] = pl.aux_base + (uint32_t)pl.aux_frame.size() * WE;
            pl.aux_frame.push_back(c | (1u << 16));
        }
    slot += (uint32_t)pl.aux_frame.size() * WE;
    pl.x_slot = x_used ? slot++ : CP_NO_SLOT;
    pl.reg_base = slot;
    pl.reg_slot.assign(prog->n_regs, CP_NO_SLOT);
    for (uint32_t r = 0; r < prog->n_regs; r++)
        if (pl.reg_type[r]) {
            pl.reg_slot[r] = slot;
            slot += pl.reg_type[r] == 2 ? WE : 1;
        }
    pl.n_slots = slot;
    pl.group_size = cp_group_size(pl.n_slots * eb);
    if (!pl.group_size && !pl.aux_frame.empty())
        return cp_fail(pl, WF_ERR_ARG, "%u frame columns, %u auxiliary frame columns of degree %u and %u register elements of %u bytes do not fit the local memory of a compute unit",
                       (uint32_t)pl.frame.size(), (uint32_t)pl.aux_frame.size(), WE, pl.reg_footprint, eb);
    if (!pl.group_size)
        return cp_fail(pl, WF_ERR_ARG, "%u frame columns and %u register elements of %u bytes do not fit the local memory of a compute unit",
                       (uint32_t)pl.frame.size(), pl.reg_footprint, eb);
    pl.lds_bytes = pl.group_size * pl.n_slots * eb;

    // ---- pass 2: the kernel's instruction form
    std::vector<uint32_t> const_off(prog->n_consts, CP_NO_SLOT), econst_off(prog->n_econsts, CP_NO_SLOT), table_ent(prog->n_tables, CP_NO_SLOT);
    pl.const_src.clear();
    pl.table_src.clear();
    pl.tables.clear();
    pl.n_const_elems = 0;
    pl.n_table_elems = 0;
    pl.instrs.resize(NI);
    for (uint32_t i = 0; i < NI; i++) {
        const wf_cprog_instr &in = prog->instrs[i];
        CpInstr &k = pl.instrs[i];
        memset(&k, 0, sizeof(k));
        k.op = (uint32_t)((in.op - 1) * 4 + typing[i]);
        k.dst = pl.reg_slot[in.dst];
        for (int o = 0; o < 2; o++) {
            const uint32_t src = o ? in.b_src : in.a_src, idx = o ? in.b : in.a;
            uint8_t kind = CPK_LDS;
            uint32_t v = 0;
            switch (src) {
                case WF_CP_REG: v = pl.reg_slot[idx]; break;
                case WF_CP_CUR: v = cur_slot[idx]; break;
                case WF_CP_NEXT: v = next_slot[idx]; break;
                case WF_CP_X: v = pl.x_slot; break;
                case WF_CP_AUX_CUR: v = aux_cur_slot[idx]; break;
                case WF_CP_AUX_NEXT: v = aux_next_slot[idx]; break;
                case WF_CP_CONST:
                    kind = CPK_CONST;
                    if (const_off[idx] == CP_NO_SLOT) {
                        const_off[idx] = pl.n_const_elems++;
                        pl.const_src.push_back(idx);
                    }
                    v = const_off[idx];
                    break;
                case WF_CP_ECONST:
                    kind = CPK_CONST;
                    if (econst_off[idx] == CP_NO_SLOT) {
                        econst_off[idx] = pl.n_const_elems;
                        pl.n_const_elems += WE;
                        pl.const_src.push_back(idx | (1u << 31));
                    }
                    v = econst_off[idx];
                    break;
                default:  // WF_CP_TABLE
                    kind = CPK_TABLE;
                    if (table_ent[idx] == CP_NO_SLOT) {
                        const wf_cprog_table &tb = prog->tables[idx];
                        if (pl.n_table_elems + ((uint64_t)1 << tb.log2_len) > 0xFFFFFFFFull)
                            return cp_fail(pl, WF_ERR_ARG, "the tables hold more than 2^32 values");
                        table_ent[idx] = (uint32_t)pl.tables.size();
                        pl.table_src.push_back(idx);
                        pl.tables.push_back(CpTable{(uint32_t)pl.n_table_elems, (uint32_t)(((uint64_t)1 << tb.log2_len) - 1), (uint32_t)tb.shift, 0});
                        pl.n_table_elems += (uint64_t)1 << tb.log2_len;
                    }
                    v = table_ent[idx];
                    break;
            }
            k.op |= (uint32_t)kind << (o ? 16 : 8);
            (o ? k.b : k.a) = v;
        }
    }
    pl.out_slot.resize(prog->n_out);
    pl.out_is_ext.resize(prog->n_out);
    for (uint32_t j = 0; j < prog->n_out; j++) {
        pl.out_slot[j] = pl.reg_slot[prog->out_regs[j]];
        pl.out_is_ext[j] = pl.reg_type[prog->out_regs[j]] == 2;
    }
    return 0;
}

inline int cprog_plan(const wf_cprog *prog, const CpShape &sh, uint32_t trace_index, uint32_t ext_degree, uint32_t log2_ce_blowup,
                      CpPlan &pl) {
    return cprog_plan_aux(prog, sh, nullptr, trace_index, 0, ext_degree, log2_ce_blowup, pl);
}

}  // namespace wf
