// swe2d_reaction.hip - reacting tracers: the swe2d_tracer_set_reaction* / swe2d_reaction_set_field entry points and the pass that
// evaluates a tracer's source program.
//
// swe_reaction_kernel<NPC> - one lane per cell, 256-lane workgroups, launched over the cell range of the stage launch it precedes -
// writes the nodal source planes of ONE tracer: at every point of the program's rule the postfix program is run on the operands
// interpolated to the point, the results are integrated against the basis functions and the reference cell's mass inverse is applied
// (include/swe2d.h has the formulas, thetis_amd/reactions.py restates them in numpy).  Everything is evaluated left to right without
// contraction, so a host replay of an arithmetic-only program has the bits of the device.
//
// The program, its constants and the rule are kernel arguments (3.1 KiB of the 4 KiB; the discrete farms pass their rule the same
// way): the opcode, the constant and phi / w are read through uniform addresses into scalar registers and every branch on an opcode
// is wave-uniform.  The operand stack would be a dynamically indexed per-lane array - scratch; it lives in LDS instead: value `sp` of
// lane l at stk[sp*256 + l] (consecutive lanes, consecutive banks: conflict-free), the topmost value in a register.  A lane reads
// and writes its own column only, so there is no barrier.  Per point and operand a lane reads the cell's NPC nodal values again
// (plane layout: coalesced, and after the first point from the cache); X / Y read the cell's vertex ids and coordinates.  Written:
// NPC doubles per cell.  No atomics, one writer per value.
#include "swe2d_handle.h"

#define SWE_RX_OPERANDS 16                      // operand table: 0..7 tracers, 8..11 coefficient fields, 12..15 free (the flow: uv, elev, depth)
#define SWE_RX_FIELD0 SWE2D_REACTION_MAX_TRACERS
static_assert(SWE_RX_FIELD0 + SWE2D_REACTION_MAX_FIELDS <= SWE_RX_OPERANDS, "operand table too small");

struct SweReactionArgs {
    const double *opnd[SWE_RX_OPERANDS];        // nodal planes [NPC][stride]
    const int *cv;                              // [NPC][stride] cell vertices
    const double *vx, *vy;
    double *source;                             // [NPC][stride]
    size_t stride;
    int cell_begin, cell_end;
    int n_code, n_q;
    int code[SWE2D_REACTION_MAX_CODE];
    double consts[SWE2D_REACTION_MAX_CONSTS];
    double phi[SWE2D_REACTION_MAX_QUAD*4];      // [n_q][NPC]
    double w[SWE2D_REACTION_MAX_QUAD];
};
static_assert(sizeof(SweReactionArgs) <= 4096, "kernel arguments beyond 4 KiB");

// an operand at a point of the rule: (phi_0 c_0 + phi_1 c_1) + phi_2 c_2 [+ phi_3 c_3]
template <int NPC>
__device__ __forceinline__ double swe_reaction_interp(const double *phi, const double c[NPC])
{
#pragma clang fp contract(off)
    double v = phi[0]*c[0] + phi[1]*c[1];
#pragma unroll
    for (int i = 2; i < NPC; i++) v = v + phi[i]*c[i];
    return v;
}

template <int NPC>
__global__ void __launch_bounds__(256) swe_reaction_kernel(SweReactionArgs a)
{
#pragma clang fp contract(off)
    __shared__ double stk[SWE2D_REACTION_MAX_STACK*256];
    const int lane = threadIdx.x;
    const int k = a.cell_begin + blockIdx.x*256 + lane;
    if (k >= a.cell_end) return;                                            // (no barrier below)
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)a.stride*8u, S4 = (unsigned)a.stride*4u;
    double b[NPC];
#pragma unroll
    for (int i = 0; i < NPC; i++) b[i] = 0.0;
    for (int q = 0; q < a.n_q; q++) {
        const double *phi = a.phi + q*NPC;
        double top = 0.0;
        int sp = 0;                                                         // values below `top`, in LDS (+ 1 unused at the bottom)
        for (int pc = 0; pc < a.n_code; pc++) {
            const int ins = a.code[pc];
            const int op = ins & 255, arg = ins >> 8;
            if (op <= SWE2D_RX_Y) {                                         // a leaf: push
                double v, c[NPC];
                if (op == SWE2D_RX_CONST) {
                    v = a.consts[arg];
                } else if (op == SWE2D_RX_X || op == SWE2D_RX_Y) {
                    const swe_rsrc_t rc = swe_rsrc(a.cv), rp = swe_rsrc(op == SWE2D_RX_X ? a.vx : a.vy);
#pragma unroll
                    for (int i = 0; i < NPC; i++) c[i] = swe_ld(rp, (unsigned)swe_ldi(rc, k4, i*S4)*8u, 0u);
                    v = swe_reaction_interp<NPC>(phi, c);
                } else {                                                    // TRACER, FIELD: a slot of the operand table
                    const swe_rsrc_t r = swe_rsrc(a.opnd[arg]);
#pragma unroll
                    for (int i = 0; i < NPC; i++) c[i] = swe_ld(r, k8, i*S8);
                    v = swe_reaction_interp<NPC>(phi, c);
                }
                stk[sp*256 + lane] = top;
                sp++;
                top = v;
            } else if (op == SWE2D_RX_NEG) { top = -top;
            } else if (op == SWE2D_RX_ABS) { top = __builtin_fabs(top);
            } else if (op == SWE2D_RX_POWI) {
                const double x = top;
                for (int j = 1; j < arg; j++) top = top*x;
            } else if (op == SWE2D_RX_SQRT) { top = sqrt(top);
            } else if (op == SWE2D_RX_EXP) { top = exp(top);
            } else if (op == SWE2D_RX_LOG) { top = log(top);
            } else if (op == SWE2D_RX_NOT) { top = top == 0.0 ? 1.0 : 0.0;
            } else if (op == SWE2D_RX_SELECT) {
                const double y = stk[(sp - 1)*256 + lane], c = stk[(sp - 2)*256 + lane];
                sp -= 2;
                top = c != 0.0 ? y : top;
            } else {                                                        // binary: x below, top above
                sp--;
                const double x = stk[sp*256 + lane];
                switch (op) {
                case SWE2D_RX_ADD: top = x + top; break;
                case SWE2D_RX_SUB: top = x - top; break;
                case SWE2D_RX_MUL: top = x*top; break;
                case SWE2D_RX_DIV: top = x/top; break;
                case SWE2D_RX_MIN: top = top < x ? top : x; break;
                case SWE2D_RX_MAX: top = top > x ? top : x; break;
                case SWE2D_RX_LT: top = x < top ? 1.0 : 0.0; break;
                case SWE2D_RX_LE: top = x <= top ? 1.0 : 0.0; break;
                case SWE2D_RX_GT: top = x > top ? 1.0 : 0.0; break;
                case SWE2D_RX_GE: top = x >= top ? 1.0 : 0.0; break;
                case SWE2D_RX_EQ: top = x == top ? 1.0 : 0.0; break;
                case SWE2D_RX_NE: top = x != top ? 1.0 : 0.0; break;
                case SWE2D_RX_AND: top = (x != 0.0 && top != 0.0) ? 1.0 : 0.0; break;
                default: top = (x != 0.0 || top != 0.0) ? 1.0 : 0.0; break;          // OR (the program was checked when it was set)
                }
            }
        }
        const double wq = a.w[q];
#pragma unroll
        for (int i = 0; i < NPC; i++) b[i] = b[i] + (wq*phi[i])*top;
    }
    const swe_rsrc_t rs = swe_rsrc(a.source);
    if constexpr (NPC == 3) {
        const double s = (b[0] + b[1]) + b[2];
#pragma unroll
        for (int i = 0; i < 3; i++) swe_st(rs, k8, i*S8, 12.0*b[i] - 3.0*s);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            swe_st(rs, k8, i*S8, (16.0*b[i] - 8.0*(b[(i + 1) & 3] + b[(i + 3) & 3])) + 4.0*b[(i + 2) & 3]);
    }
}

namespace {

int reaction_check(Handle *h, int id)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (id < 0 || id >= (int)h->tracers.size()) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "unknown tracer id");
    return SWE2D_OK;
}

}  // namespace

int swe2d_impl::reaction_launch(Handle *h, int id, int in, int c0, int c1)
{
    Handle::Tracer &t = h->tracers[id];
    const Handle::Tracer::Reaction &rx = t.rx;
    if (c1 <= c0 || rx.n_code <= 0) return SWE2D_OK;
    if (!t.source) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "reaction: the tracer has no source planes");
    if (h->npc == 4 && !h->affine)
        return fail(h, SWE2D_ERR_UNSUPPORTED, "reaction programs are evaluated on triangles and parallelograms only (general quadrilaterals: the Jacobian varies)");
    SweReactionArgs a{};
    for (int s = 0; s < rx.n_tracers; s++) {
        const int j = rx.tracer_ids[s];
        if (j < 0 || j >= (int)h->tracers.size()) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "reaction: unknown tracer operand");
        // the stage's own input for the tracer being stepped, buffer A (already stepped / still old) for every other tracer
        a.opnd[s] = h->tracers[j].buf[j == id ? in : 0];
    }
    for (int f = 0; f < SWE2D_REACTION_MAX_FIELDS; f++) {
        if (((rx.field_mask >> f) & 1u) && !h->rx_field[f])
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "reaction: coefficient field " + std::to_string(f) + " is not set (swe2d_reaction_set_field)");
        a.opnd[SWE_RX_FIELD0 + f] = h->rx_field[f];
    }
    a.cv = h->cv; a.vx = h->vx; a.vy = h->vy;
    a.source = t.source;
    a.stride = h->stride;
    a.cell_begin = c0; a.cell_end = c1;
    a.n_code = rx.n_code; a.n_q = rx.n_q;
    std::memcpy(a.code, rx.code, sizeof(a.code));
    std::memcpy(a.consts, rx.consts, sizeof(a.consts));
    std::memcpy(a.phi, rx.phi, sizeof(a.phi));
    std::memcpy(a.w, rx.w, sizeof(a.w));
    SWE_CHK_SYNC(h->stream);
    const dim3 grid((unsigned)grid_for(c1 - c0));
    if (h->npc == 4) hipLaunchKernelGGL(swe_reaction_kernel<4>, grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(swe_reaction_kernel<3>, grid, dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

extern "C" {

int swe2d_tracer_set_reaction(swe2d_handle *hh, int id, int32_t n_code, const int32_t *code, int32_t n_const, const double *consts,
                              int32_t n_q, const double *phi, const double *w)
{
    Handle *h = H(hh);
    if (int rc = reaction_check(h, id)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    Handle::Tracer &t = h->tracers[id];
    if (h->sed.on && id == h->sed.tracer)
        return n_code == 0 ? SWE2D_OK : fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction: the sediment field's source comes from the sediment model (swe2d_sediment_clear first)");
    if (n_code == 0) {                                                      // no program, no source
        t.rx.n_code = 0;
        if (t.source) { HIP_TRY(h, hipStreamSynchronize(h->stream)); t.source.reset(); }
        return SWE2D_OK;
    }
    if (h->npc == 4 && !h->affine)
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_tracer_set_reaction: triangles and parallelograms only (general quadrilaterals: the Jacobian varies)");
    if (n_code < 0 || n_code > SWE2D_REACTION_MAX_CODE || !code)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction: n_code must be in 0 .. SWE2D_REACTION_MAX_CODE");
    if (n_const < 0 || n_const > SWE2D_REACTION_MAX_CONSTS || (n_const > 0 && !consts))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction: n_const must be in 0 .. SWE2D_REACTION_MAX_CONSTS");
    if (n_q < 1 || n_q > SWE2D_REACTION_MAX_QUAD || !phi || !w)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction: n_q must be in 1 .. SWE2D_REACTION_MAX_QUAD");
    for (int i = 0; i < n_q*h->npc; i++)
        if (!std::isfinite(phi[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction: the rule must be finite");
    for (int i = 0; i < n_q; i++)
        if (!std::isfinite(w[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction: the rule must be finite");
    // the program on a stack of depths: every operand in range, no underflow, never more than the LDS columns hold, one value left
    Handle::Tracer::Reaction rx;
    int depth = 0;
    for (int pc = 0; pc < n_code; pc++) {
        const int op = code[pc] & 255, arg = (int)((unsigned)code[pc] >> 8);
        int pops = 0, pushes = 1, arg_out = 0;
        const std::string at = "swe2d_tracer_set_reaction: instruction " + std::to_string(pc) + ": ";
        if (op < 0 || op >= SWE2D_RX_COUNT) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "unknown opcode");
        if (op == SWE2D_RX_CONST) {
            if (arg >= n_const) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "constant out of range");
            arg_out = arg;
        } else if (op == SWE2D_RX_TRACER) {
            if (arg >= (int)h->tracers.size()) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "unknown tracer");
            int s = 0;
            while (s < rx.n_tracers && rx.tracer_ids[s] != arg) s++;
            if (s == rx.n_tracers) {
                if (s == SWE2D_REACTION_MAX_TRACERS)
                    return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "more than SWE2D_REACTION_MAX_TRACERS distinct tracers");
                rx.tracer_ids[rx.n_tracers++] = arg;
            }
            arg_out = s;
        } else if (op == SWE2D_RX_FIELD) {
            if (arg >= SWE2D_REACTION_MAX_FIELDS) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "coefficient field out of range");
            rx.field_mask |= 1u << arg;
            arg_out = SWE_RX_FIELD0 + arg;
        } else if (op == SWE2D_RX_X || op == SWE2D_RX_Y) {
        } else if (op == SWE2D_RX_NEG || op == SWE2D_RX_ABS || op == SWE2D_RX_SQRT || op == SWE2D_RX_EXP || op == SWE2D_RX_LOG
                   || op == SWE2D_RX_NOT) {
            pops = 1;
        } else if (op == SWE2D_RX_POWI) {
            if (arg < 2 || arg > 16) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "POWI takes 2 <= n <= 16");
            pops = 1; arg_out = arg;
        } else if (op == SWE2D_RX_SELECT) {
            pops = 3;
        } else {
            pops = 2;
        }
        if (depth < pops) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "stack underflow");
        depth += pushes - pops;
        if (depth > SWE2D_REACTION_MAX_STACK) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, at + "more than SWE2D_REACTION_MAX_STACK values on the stack");
        rx.code[pc] = op | (arg_out << 8);
    }
    if (depth != 1) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction: the program must leave exactly one value");
    rx.n_code = n_code; rx.n_const = n_const; rx.n_q = n_q;
    for (int i = 0; i < n_const; i++) rx.consts[i] = consts[i];
    std::memcpy(rx.phi, phi, (size_t)n_q*h->npc*sizeof(double));
    std::memcpy(rx.w, w, (size_t)n_q*sizeof(double));
    if (!t.source) {
        const size_t bytes = (size_t)h->npc*h->stride*sizeof(double);
        HIP_TRY(h, t.source.alloc(bytes/sizeof(double)));
        HIP_TRY(h, hipMemsetAsync(t.source, 0, bytes, h->stream));
    }
    t.rx = rx;
    return SWE2D_OK;
}

int swe2d_tracer_set_reaction_constants(swe2d_handle *hh, int id, int32_t n_const, const double *consts)
{
    Handle *h = H(hh);
    if (int rc = reaction_check(h, id)) return rc;
    Handle::Tracer::Reaction &rx = h->tracers[id].rx;
    if (rx.n_code <= 0) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction_constants: the tracer has no program");
    if (n_const != rx.n_const || (n_const > 0 && !consts))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_set_reaction_constants: n_const differs from the program's");
    for (int i = 0; i < n_const; i++) rx.consts[i] = consts[i];             // (kernel arguments of the launches from now on)
    return SWE2D_OK;
}

int swe2d_reaction_set_field(swe2d_handle *hh, int32_t slot, const double *nodal)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (slot < 0 || slot >= SWE2D_REACTION_MAX_FIELDS) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_reaction_set_field: slot out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!nodal) {
        if (h->rx_field[slot]) { HIP_TRY(h, hipStreamSynchronize(h->stream)); h->rx_field[slot].reset(); }
        return SWE2D_OK;
    }
    if (!h->rx_field[slot]) {
        const size_t bytes = (size_t)h->npc*h->stride*sizeof(double);
        HIP_TRY(h, h->rx_field[slot].alloc(bytes/sizeof(double)));
        HIP_TRY(h, hipMemsetAsync(h->rx_field[slot], 0, bytes, h->stream));          // (the planes' padding beyond n_cells)
    }
    HIP_TRY(h, hipMemcpyAsync(h->stage_eta, nodal, (size_t)h->npc*h->n_cells*sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(swe_nodal_to_planes, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream,
                       h->stage_eta, h->rx_field[slot], h->stride, h->n_cells, 1, h->npc);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

int swe2d_tracer_get_source(swe2d_handle *hh, int id, double *nodal)
{
    Handle *h = H(hh);
    if (int rc = reaction_check(h, id)) return rc;
    if (!nodal) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (!h->tracers[id].source) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_get_source: the tracer has no source");
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream,
                       h->tracers[id].source, h->stage_eta, h->stride, h->n_cells, h->npc);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(nodal, h->stage_eta, (size_t)h->npc*h->n_cells*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

int swe2d_tracer_get_buffer(swe2d_handle *hh, int id, int i_buffer, double *nodal)
{
    Handle *h = H(hh);
    if (int rc = reaction_check(h, id)) return rc;
    if (!nodal || i_buffer < 0 || i_buffer > 2) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tracer_get_buffer: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream,
                       h->tracers[id].buf[i_buffer], h->stage_eta, h->stride, h->n_cells, h->npc);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(nodal, h->stage_eta, (size_t)h->npc*h->n_cells*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

}  // extern "C"
