// packed_launch.h — "pack, upload, run, read back": the host sequence shared by the single-phase entry points
// whose kernels read a struct of device pointers per problem (fuse.hip, sim3.hip, triang.hip, init.hip,
// stereo.hip).  The inputs are an osg_packer's items, each bound to the pointer field that is to receive its
// device address (match_common.h); batch_io.h is the counterpart for arrays concatenated over the batch.
//
//   osg_packer pk;
//   std::vector<Args> args(B);                 // sized before the first bind: bindings hold field addresses
//   pk.bind(args[b].x, src, bytes); ...        // per problem
//   osg_packed_launch L(ctx, pk);
//   OSG_RC(L.stage(sizeof(Args) * B, out_bytes));   // pinned block [in | args | out], the stream idle, the fill
//   OSG_RC(L.alloc());                         // SLOT_TMP0 / 1 / 2; every bound field now a device address
//   args[b].out = L.dev_out<int32_t>() + ...;  // output and scratch pointers (further slots are the caller's)
//   OSG_RC(L.upload(args.data()));             // inputs, then arguments
//   OSG_RC(L.start());                         // ev[0]
//   launches on ctx->stream with L.dev_args<Args>()
//   OSG_RC(L.finish());                        // hipGetLastError, ev[1], download, wait, ctx->last_kernel_ms
//   L.out<int32_t>()                           // the downloaded output block
//
// A unit that passes its arguments by value has no args block: stage(0, out_bytes), upload(nullptr), and
// SLOT_TMP1 is not touched.  stage() and finish() are each two steps (reserve + fill, download + wait) that a
// unit timing its host phases calls one by one.
#pragma once
#include <cstring>

#include "match_common.h"

struct osg_packed_launch {
    osg_ctx *ctx;
    const osg_packer &pk;
    size_t in_bytes = 0, args_bytes = 0, args_pad = 0, out_bytes = 0;
    char *pin = nullptr, *din = nullptr, *dargs = nullptr, *dout = nullptr;
    hipEvent_t *ev = nullptr;  // the context's two timing events, around the launches
    float kernel_ms = 0.f;

    osg_packed_launch(osg_ctx *c, const osg_packer &p) : ctx(c), pk(p) {}

    int reserve(size_t args_bytes_, size_t out_bytes_)
    {
        in_bytes = (pk.total + 255) & ~size_t(255);
        args_bytes = args_bytes_;
        args_pad = (args_bytes + 255) & ~size_t(255);
        out_bytes = out_bytes_;
        pin = (char *)osg_pinned(ctx, in_bytes + args_pad + out_bytes + 256);
        if (!pin) return osg_set_error(ctx, OSG_E_NOMEM, "pinned alloc failed");
        return osg_idle(ctx);  // the pinned block may still be in use
    }
    void fill(bool parallel) const
    {
        if (parallel) pk.fill_parallel(pin, 8);
        else pk.fill(pin);
    }
    int stage(size_t args_bytes_, size_t out_bytes_, bool parallel = true)
    {
        OSG_RC(reserve(args_bytes_, out_bytes_));
        fill(parallel);
        return 0;
    }
    int alloc()
    {
        OSG_ALLOC(ctx, din, SLOT_TMP0, pk.total + 256);
        if (args_bytes) OSG_ALLOC(ctx, dargs, SLOT_TMP1, args_pad);
        OSG_ALLOC(ctx, dout, SLOT_TMP2, out_bytes);
        pk.relocate(din);
        return 0;
    }
    template <class T>
    T *dev_args() const
    {
        return (T *)dargs;
    }
    template <class T>
    T *dev_out() const
    {
        return (T *)dout;
    }
    // args: the B argument structs, complete (copied into the pinned block first); nullptr without an args block
    int upload(const void *args)
    {
        if (pk.total) OSG_HIP_CHECK(ctx, hipMemcpyAsync(din, pin, pk.total, hipMemcpyHostToDevice, ctx->stream));
        if (!args_bytes) return 0;
        std::memcpy(pin + in_bytes, args, args_bytes);
        OSG_HIP_CHECK(ctx, hipMemcpyAsync(dargs, pin + in_bytes, args_bytes, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    int start()
    {
        ev = osg_ctx_events(ctx);
        if (!ev) return osg_set_error(ctx, OSG_E_HIP, "event create failed");
        OSG_HIP_CHECK(ctx, hipEventRecord(ev[0], ctx->stream));
        return 0;
    }
    int download()
    {
        OSG_HIP_CHECK(ctx, hipGetLastError());  // the last launch's
        OSG_HIP_CHECK(ctx, hipEventRecord(ev[1], ctx->stream));
        return osg_download(ctx, pin + in_bytes + args_pad, dout, out_bytes);
    }
    int wait()
    {
        OSG_RC(osg_wait(ctx));
        OSG_HIP_CHECK(ctx, hipEventElapsedTime(&kernel_ms, ev[0], ev[1]));
        ctx->last_kernel_ms = kernel_ms;
        return 0;
    }
    int finish()
    {
        OSG_RC(download());
        return wait();
    }
    // the output block, as downloaded
    template <class T>
    const T *out() const
    {
        return (const T *)(pin + in_bytes + args_pad);
    }
};
