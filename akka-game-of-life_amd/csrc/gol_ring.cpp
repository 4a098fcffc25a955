// gol_ring.cpp -- the ring schedule of a sharded context: one pass of G
// generations = the interior rows' launch || a G-deep halo exchange with the
// ring neighbours (one RCCL send/recv group on the comm stream, or the
// in-process loopback ring of gol_loopback.cpp that tests use in its place),
// then the boundary rows.  A context stepped whole runs whole_pass
// (gol_active.cpp) instead.
// Replaces the cross-backend GetStateFromEpoch / StateForEpoch traffic
// of the reference (CellActor.scala:71-77, NextStateCellGathererActor.scala:32-36).
#include <cstring>

#include "gol_ctx.h"

using namespace golc;

namespace {

// A pass's halo operations as one RCCL group on the comm stream.
int rccl_exchange(gol_ctx* ctx, const HaloOp* ops, int nops) {
    NCCL_CHECK(ctx, ncclGroupStart());
    for (int k = 0; k < nops; ++k) {
        if (ops[k].send)
            NCCL_CHECK(ctx, ncclSend(ops[k].buf, ops[k].count, ncclUint32, ops[k].peer, ctx->nccl, ctx->comm));
        else
            NCCL_CHECK(ctx, ncclRecv(ops[k].buf, ops[k].count, ncclUint32, ops[k].peer, ctx->nccl, ctx->comm));
    }
    NCCL_CHECK(ctx, ncclGroupEnd());
    return GOL_OK;
}

}  // namespace

namespace golc {

// One pass of G generations (temporal blocking, G <= kMaxGensPerPass) of a
// stand-alone or RCCL-sharded context, summing what `sums` says.
int one_pass(gol_ctx* ctx, int G, PassSums sums) {
    uint32_t* cur = ctx->plane[ctx->cur];
    uint32_t* nxt = ctx->plane[ctx->cur ^ 1];
    const int32_t rows = (int32_t)ctx->rows;
    const bool torus = ctx->topology == GOL_TORUS;
    const int64_t pitch = ctx->pitch;
    if (!sharded(ctx)) {
        // torus: rows wrap inside the plane; clipped: outside rows are dead
        PassLaunch L;
        L.gens = G;
        L.cur = cur;
        L.nxt = nxt;
        L.halo_top = L.halo_bot = ctx->zero_row;
        L.wrap_y = torus;
        L.sums = sums;
        if (int rc = whole_pass(ctx, L)) return rc;
    } else if (ctx->group) {
        return set_err(ctx, GOL_ESTATE, "context belongs to a shard group: step it with gol_group_step");
    } else {
        live_unknown(ctx, 0);  // a sharded pass runs dense: active-row stepping covers contexts stepped whole only
        live_unknown(ctx, 1);
        const int up = (ctx->rank + ctx->nranks - 1) % ctx->nranks;
        const int down = (ctx->rank + 1) % ctx->nranks;
        const bool has_up = torus || ctx->rank > 0;
        const bool has_down = torus || ctx->rank < ctx->nranks - 1;
        // profiling (null: off): the interior launch, the exchange and the boundary launch bracket their parts
        PassRecord* rec = nullptr;
        HIP_CHECK(ctx, ctx->profile.begin(&rec, ctx->compute));
        // G-deep halo exchange on the comm stream once the current plane is
        // final (ev_ready: recorded before this pass's interior launch, so the
        // exchange does not wait for it).  The interior launch is enqueued
        // first: the GPU starts it while the host is still inside the RCCL
        // group calls.  If it cannot be enqueued, the halo operations are
        // still posted before the error is returned: the peers' groups then
        // complete instead of blocking in ncclGroupEnd until someone aborts
        // the communicator.
        HIP_CHECK(ctx, hipEventRecord(ctx->ev_ready, ctx->compute));
        const int rc_interior = sharded_interior(ctx, G, sums, has_up, has_down, rec);
        HIP_CHECK(ctx, hipStreamWaitEvent(ctx->comm, ctx->ev_ready, 0));
        const size_t cnt = (size_t)G * pitch;  // G contiguous rows (pitch padding included)
        // Issue order matters when up == down (2 ranks, or 1 rank sending to
        // itself): per-peer FIFO matching pairs my last rows with the peer's
        // top halo and my first rows with its bottom halo
        // (gameoflife/shard.py HaloPlan mirrors this order).  One op list,
        // run by RCCL or by the in-process loopback ring.
        HaloOp ops[4];
        int nops = 0;
        if (has_down) ops[nops++] = {true, cur + (int64_t)(rows - G) * pitch, cnt, down};
        if (has_up) ops[nops++] = {true, cur, cnt, up};
        if (has_up) ops[nops++] = {false, ctx->halo_top, cnt, up};
        if (has_down) ops[nops++] = {false, ctx->halo_bot, cnt, down};
        // exchange timing (gol_profile_stats): comm-stream events around the group; a part left without its
        // stop (a failed exchange) is skipped by the fold
        if (rec && rc_interior == GOL_OK) HIP_CHECK(ctx, ctx->profile.start(rec, kProfExchange, ctx->comm));
        gol_profile_stats& t = ctx->profile.totals.stats;
        for (int k = 0; k < nops; ++k) (ops[k].send ? t.halo_bytes_sent : t.halo_bytes_received) += ops[k].count * 4;
        const int rc_x = ctx->loop ? loop_exchange(ctx, ops, nops) : rccl_exchange(ctx, ops, nops);
        if (rec && rc_x == GOL_OK) HIP_CHECK(ctx, ctx->profile.stop(rec, kProfExchange, ctx->comm));
        if (rc_interior) return rc_interior;
        if (rc_x) return rc_x;
        // The event covers the sends too: the next pass overwrites this plane
        // only after the boundary kernels, which wait for it.
        HIP_CHECK(ctx, hipEventRecord(ctx->ev_halo, ctx->comm));
        if (int rc = sharded_boundary(ctx, G, sums, has_up, has_down, &ctx->ev_halo, 1, rec)) return rc;
    }
    ctx->cur ^= 1;
    ctx->epoch += (uint64_t)G;
    return GOL_OK;
}

}  // namespace golc

extern "C" {

int gol_comm_abort(gol_ctx* ctx) {
    if (!ctx) return set_err(nullptr, GOL_EINVAL, "null context");
    if (ctx->loop) {
        if (int rc = bind(ctx)) return rc;
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->comm));
        loop_leave(ctx);
        ctx->rank = 0;
        ctx->nranks = 1;
        return GOL_OK;
    }
    if (!ctx->nccl) return GOL_OK;
    if (int rc = bind(ctx)) return rc;
    NCCL_CHECK(ctx, ncclCommAbort(ctx->nccl));
    ctx->nccl = nullptr;
    ctx->rank = 0;
    ctx->nranks = 1;
    return GOL_OK;
}

int gol_comm_unique_id(uint8_t id_out[GOL_UNIQUE_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == GOL_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!id_out) return set_err(nullptr, GOL_EINVAL, "null argument");
    ncclUniqueId id;
    NCCL_CHECK(nullptr, ncclGetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return GOL_OK;
}

int gol_comm_init(gol_ctx* ctx, const uint8_t id[GOL_UNIQUE_ID_BYTES], int rank, int nranks) {
    if (!ctx || !id) return set_err(ctx, GOL_EINVAL, "null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return set_err(ctx, GOL_EINVAL, "bad rank/nranks");
    if (in_ring(ctx)) return set_err(ctx, GOL_ESTATE, "communicator already initialised");
    if (int rc = bind(ctx)) return rc;
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    NCCL_CHECK(ctx, ncclCommInitRank(&ctx->nccl, nranks, uid, rank));
    ctx->rank = rank;
    ctx->nranks = nranks;
    return GOL_OK;
}

int gol_comm_allreduce_u64(gol_ctx* ctx, uint64_t* values, uint32_t count) {
    if (!ctx || (!values && count)) return set_err(ctx, GOL_EINVAL, "null argument");
    if (!in_ring(ctx)) return set_err(ctx, GOL_ECOMM, "no communicator (call gol_comm_init)");
    if (count == 0) return GOL_OK;
    if (ctx->loop) return loop_allreduce(ctx, values, count);
    if (int rc = bind(ctx)) return rc;
    uint64_t* d = nullptr;
    HIP_CHECK(ctx, hipMallocAsync((void**)&d, count * sizeof(uint64_t), ctx->comm));
    HIP_CHECK(ctx, hipMemcpyAsync(d, values, count * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->comm));
    NCCL_CHECK(ctx, ncclAllReduce(d, d, count, ncclUint64, ncclSum, ctx->nccl, ctx->comm));
    HIP_CHECK(ctx, hipMemcpyAsync(values, d, count * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->comm));
    HIP_CHECK(ctx, hipFreeAsync(d, ctx->comm));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->comm));
    return GOL_OK;
}

}  // extern "C"
