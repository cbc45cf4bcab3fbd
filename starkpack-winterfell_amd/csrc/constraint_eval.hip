// libwf_lde.so, unit 8 of 8 -- constraint programs: ConstraintEvaluator::evaluate (prover/src/constraints/evaluator.rs:74-241)
// on the resident trace LDE: the main segment alone (wf_constraint_evaluate) or the main and the auxiliary segment
// (wf_constraint_evaluate_aux: evaluate_fragment_full, :190-241).  The host side plans the caller's program (cprog_plan.hpp), uploads
// its kernel form in one piece and launches the interpreter (cprog_kernels.hpp); the evaluation columns stay in device memory
// (wf_evaluations) for wf_constraint_commit_from_device_tables (path.hip).
#include "wf_internal.hpp"

#include "cprog_kernels.hpp"
#include "tables.hpp"

using namespace wf;

static void free_evaluations(wf_evaluations *e) {
    if (!e) return;
    if (ctx_alive(e->ctx, e->ctx_generation)) (void)hipSetDevice(e->ctx->device);
    if (e->uploaded) {  // the queued upload reads the pinned image: it must have left before the image is freed
        (void)hipEventSynchronize(e->uploaded);  // (the event is the handle's own: no context needed to wait for it)
        (void)hipEventDestroy(e->uploaded);
    }
    if (e->prog_host) (void)hipHostFree(e->prog_host);
    pool_free(e->ctx, e->ctx_generation, e->cols, e->cols_bytes);
    pool_free(e->ctx, e->ctx_generation, e->prog, e->prog_bytes);
    delete e;
}

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

template <class F, int WE>
static int evaluate_dev(wf_ctx *ctx, hipStream_t st, const wf_commitment *c, uint32_t trace_index, const wf_commitment *aux,
                        uint32_t aux_index, const wf_cprog *prog, const CpPlan &pl, wf_evaluations *e) {
    typedef typename F::T T;
    const size_t eb = sizeof(T);
    // the program as the kernel reads it, one upload: instructions | frame | outputs | table descriptors | constants | tables
    // | aux frame (last: a program without auxiliary sources is uploaded as it always was)
    const size_t o_instr = 0, o_frame = align16(o_instr + pl.instrs.size() * sizeof(CpInstr));
    const size_t o_outs = align16(o_frame + pl.frame.size() * 4), o_tdesc = align16(o_outs + pl.out_slot.size() * 4);
    const size_t o_const = align16(o_tdesc + pl.tables.size() * sizeof(CpTable)), o_tval = align16(o_const + pl.n_const_elems * eb);
    const size_t o_aux = align16(o_tval + pl.n_table_elems * eb);
    const size_t total = align16(o_aux + pl.aux_frame.size() * 4);
    HIP_TRY(hipHostMalloc(&e->prog_host, total, hipHostMallocDefault));
    unsigned char *h = (unsigned char *)e->prog_host;
    memset(h, 0, total);
    memcpy(h + o_instr, pl.instrs.data(), pl.instrs.size() * sizeof(CpInstr));
    if (!pl.frame.empty()) memcpy(h + o_frame, pl.frame.data(), pl.frame.size() * 4);
    for (size_t j = 0; j < pl.out_slot.size(); j++) {
        const uint32_t o = pl.out_slot[j] | (pl.out_is_ext[j] ? 1u << 31 : 0u);
        memcpy(h + o_outs + j * 4, &o, 4);
    }
    if (!pl.aux_frame.empty()) memcpy(h + o_aux, pl.aux_frame.data(), pl.aux_frame.size() * 4);
    if (!pl.tables.empty()) memcpy(h + o_tdesc, pl.tables.data(), pl.tables.size() * sizeof(CpTable));
    {
        size_t off = o_const;
        for (uint32_t src : pl.const_src) {
            const bool is_e = src >> 31;
            const size_t idx = src & 0x7FFFFFFFu, nb = is_e ? WE * eb : eb;
            memcpy(h + off, (const char *)(is_e ? prog->econsts : prog->consts) + idx * nb, nb);
            off += nb;
        }
    }
    for (size_t t = 0; t < pl.tables.size(); t++)
        memcpy(h + o_tval + (size_t)pl.tables[t].offset * eb, prog->tables[pl.table_src[t]].values, ((size_t)pl.tables[t].mask + 1) * eb);

    TableSet *tw;
    int rc;
    if ((rc = root_tables<F>(ctx, c->p.log2_trace_len + c->p.log2_blowup - pl.lde_shift, false, &tw))) return rc;
    hipError_t err;
    e->cols_bytes = (size_t)e->n_columns * pl.ce * WE * eb;
    e->prog_bytes = total;
    if ((err = pool_alloc(ctx, &e->cols, e->cols_bytes)) != hipSuccess || (err = pool_alloc(ctx, &e->prog, e->prog_bytes)) != hipSuccess)
        return fail(WF_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(err));
    HIP_TRY(hipEventCreateWithFlags(&e->uploaded, hipEventDisableTiming));
    HIP_TRY(hipMemcpyAsync(e->prog, h, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e->uploaded, st));

    CprogArgs<F> a;
    memset(&a, 0, sizeof(a));
    const char *d = (const char *)e->prog;
    a.lde = (const T *)c->lde + (size_t)trace_index * c->n_rows * c->row_width;
    a.out = (T *)e->cols;
    a.instrs = (const CpInstr *)(d + o_instr);
    a.frame = (const uint32_t *)(d + o_frame);
    a.outs = (const uint32_t *)(d + o_outs);
    a.tables = (const CpTable *)(d + o_tdesc);
    a.consts = (const T *)(d + o_const);
    a.table_values = (const T *)(d + o_tval);
    a.ce = pl.ce;
    a.n_mask = c->n_rows - 1;
    a.next_rows = (uint64_t)1 << c->p.log2_blowup;
    a.n_instrs = (uint32_t)pl.instrs.size();
    a.n_frame = (uint32_t)pl.frame.size();
    a.n_out = e->n_columns;
    a.x_slot = pl.x_slot;
    a.lde_shift = pl.lde_shift;
    a.row_width = (uint32_t)c->row_width;
    u128 off;
    memcpy(&off, c->p.domain_offset, 16);
    a.offset = F::from_u128_canonical(off);
    a.g = as_pow2l<F>(*tw);
    const dim3 grid((uint32_t)((pl.ce + pl.group_size - 1) / pl.group_size)), block(pl.group_size);
    if (pl.aux_frame.empty()) {  // nothing is read from the auxiliary segment: the main kernel
        if (pl.lds_bytes > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)k_cprog_eval<F, WE>, hipFuncAttributeMaxDynamicSharedMemorySize, CP_LDS_BYTES));
        prof_mark(ctx, st, "constraint.evaluate");
        hipLaunchKernelGGL((k_cprog_eval<F, WE>), grid, block, pl.lds_bytes, st, a);
    } else {
        CprogAuxArgs<F> x;
        memset(&x, 0, sizeof(x));
        x.lde = (const T *)aux->lde + (size_t)aux_index * aux->n_rows * aux->row_width;
        x.frame = (const uint32_t *)(d + o_aux);
        x.n_frame = (uint32_t)pl.aux_frame.size();
        x.base = pl.aux_base;
        x.row_width = (uint32_t)aux->row_width;
        if (pl.lds_bytes > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)k_cprog_eval_aux<F, WE>, hipFuncAttributeMaxDynamicSharedMemorySize, CP_LDS_BYTES));
        prof_mark(ctx, st, "constraint.evaluate_aux");
        hipLaunchKernelGGL((k_cprog_eval_aux<F, WE>), grid, block, pl.lds_bytes, st, a, x);
    }
    HIP_TRY(hipGetLastError());
    prof_mark(ctx, st, "between_calls");
    return 0;
}

static CpShape shape_of(const wf_commitment *c) {
    CpShape sh;
    sh.field = c->p.field;
    sh.trace_ext = c->p.ext_degree;
    sh.n_cols = c->p.n_cols;
    sh.n_traces = c->p.n_traces;
    sh.log2_trace_len = c->p.log2_trace_len;
    sh.log2_blowup = c->p.log2_blowup;
    sh.has_lde = c->lde != nullptr && c->row_width >= (uint64_t)c->p.n_cols * c->p.ext_degree;
    return sh;
}

// both entry points; aux == nullptr: the main segment only
static int evaluate(const wf_commitment *trace, uint32_t trace_index, const wf_commitment *aux, uint32_t aux_index, const wf_cprog *prog,
                    uint32_t ext_degree, uint32_t log2_ce_blowup, wf_evaluations **out) {
    const CpShape sh = shape_of(trace);
    CpShape sh_aux;
    if (aux) sh_aux = shape_of(aux);
    CpPlan pl;
    int rc = cprog_plan_aux(prog, sh, aux ? &sh_aux : nullptr, trace_index, aux_index, ext_degree, log2_ce_blowup, pl);
    if (rc) return fail(rc, "%s", pl.msg);
    wf_ctx *ctx = trace->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    WF_ENTER(ctx, st);
    wf_evaluations *e = new wf_evaluations();
    e->ctx = ctx;
    e->ctx_generation = ctx->generation;
    e->device = ctx->device;
    e->field = sh.field;
    e->ext = ext_degree;
    e->n_columns = prog->n_out;
    e->ce = pl.ce;
    if (sh.field == WF_FIELD_F64)
        rc = ext_degree == 1   ? evaluate_dev<F64, 1>(ctx, st, trace, trace_index, aux, aux_index, prog, pl, e)
             : ext_degree == 2 ? evaluate_dev<F64, 2>(ctx, st, trace, trace_index, aux, aux_index, prog, pl, e)
                               : evaluate_dev<F64, 3>(ctx, st, trace, trace_index, aux, aux_index, prog, pl, e);
    else
        rc = ext_degree == 1 ? evaluate_dev<F128, 1>(ctx, st, trace, trace_index, aux, aux_index, prog, pl, e)
                             : evaluate_dev<F128, 2>(ctx, st, trace, trace_index, aux, aux_index, prog, pl, e);
    if (rc) {
        (void)hipStreamSynchronize(st);  // whatever was queued into the handle's buffers has drained before they go away
        free_evaluations(e);
        return rc;
    }
    *out = e;
    return 0;
}

extern "C" {

int wf_constraint_evaluate(const wf_commitment *trace, uint32_t trace_index, const wf_cprog *prog, uint32_t ext_degree,
                           uint32_t log2_ce_blowup, wf_evaluations **out) {
    if (!trace) return fail(WF_ERR_ARG, "commitment is null");
    if (!out) return fail(WF_ERR_ARG, "out is null");
    return evaluate(trace, trace_index, nullptr, 0, prog, ext_degree, log2_ce_blowup, out);
}

int wf_constraint_evaluate_aux(const wf_commitment *main_trace, uint32_t main_index, const wf_commitment *aux_trace, uint32_t aux_index,
                               const wf_cprog *prog, uint32_t ext_degree, uint32_t log2_ce_blowup, wf_evaluations **out) {
    if (!main_trace) return fail(WF_ERR_ARG, "main commitment is null");
    if (!aux_trace) return fail(WF_ERR_ARG, "auxiliary commitment is null");
    if (!out) return fail(WF_ERR_ARG, "out is null");
    if (aux_trace->ctx != main_trace->ctx || aux_trace->ctx_generation != main_trace->ctx_generation)
        return fail(WF_ERR_ARG, "the auxiliary commitment belongs to another context");
    if (memcmp(aux_trace->p.domain_offset, main_trace->p.domain_offset, sizeof(main_trace->p.domain_offset)))
        return fail(WF_ERR_ARG, "the auxiliary commitment's domain_offset differs from the main commitment's");
    return evaluate(main_trace, main_index, aux_trace, aux_index, prog, ext_degree, log2_ce_blowup, out);
}

int wf_evaluations_info(const wf_evaluations *e, uint32_t *n_columns, uint64_t *ce_domain_size, uint32_t *ext_degree) {
    if (!e) return fail(WF_ERR_ARG, "evaluations handle is null");
    if (n_columns) *n_columns = e->n_columns;
    if (ce_domain_size) *ce_domain_size = e->ce;
    if (ext_degree) *ext_degree = e->ext;
    return 0;
}

int wf_evaluations_read(const wf_evaluations *e, uint32_t column, void *out) {
    if (!e) return fail(WF_ERR_ARG, "evaluations handle is null");
    if (!out) return fail(WF_ERR_ARG, "out is null");
    if (column >= e->n_columns) return fail(WF_ERR_ARG, "column %u of %u", column, e->n_columns);
    wf_ctx *ctx = e->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    WF_ENTER(ctx, ctx->stream);
    const size_t colb = (size_t)e->ce * e->ext * wf_elem_bytes(e->field);
    HIP_TRY(hipMemcpyAsync(out, (const char *)e->cols + (size_t)column * colb, colb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

void wf_evaluations_destroy(wf_evaluations *e) { free_evaluations(e); }

}  // extern "C"
