// batch_io.h — "pack a batch, run, read back": the host sequence shared by the batch entry points of
// sim3ransac.hip, mlpnp.hip, twoview.hip and sim3opt.hip.
//
// An entry point concatenates each of its arrays over the problems of the batch (the kernels index them with
// per-problem element offsets), so a segment here is one such array, not one problem's piece of it; that is
// why this is not an osg_packer, whose items are 256-byte aligned one by one.  The layout is declared once,
// as (element bytes, count) pairs, and the copy-in, the kernel arguments and the copy-back all read a
// segment's offset and element size from the same osg_seg.
//
//   osg_batch_io io(ctx);
//   const osg_seg s_x = io.in(12, n_pts), ..., s_y = io.out(4, n_hyp), ...;   // layout
//   OSG_RC(io.stage());                        // pinned block [in | out]; the stream is idle
//   io.put(s_x, first, src, count); ...        // copy-in
//   OSG_RC(io.upload());                       // device blocks (SLOT_BA0, SLOT_BA1), one upload
//   OSG_RC(io.start());                        // ev[0]
//   launches on ctx->stream with io.dev_in<T>(s_x), io.dev_out<T>(s_y)
//   OSG_RC(io.finish(dl_bytes));               // ev[1], one download of the first dl_bytes of the output
//                                              // block, wait, ctx->last_kernel_ms
//   io.get(dst, s_y, first, count); ...        // copy-back
#pragma once
#include <cstring>

#include "osg_internal.h"

// a 256-byte-aligned segment of a block: where it starts and how large one element is
struct osg_seg {
    size_t off, elem;
};

// appends a segment of count elements to a block of `bytes` bytes
inline osg_seg osg_seg_add(size_t &bytes, size_t elem, size_t count)
{
    const osg_seg s = {bytes, elem};
    bytes += (elem * count + 255) & ~size_t(255);
    return s;
}

struct osg_batch_io {
    osg_ctx *ctx;
    size_t in_bytes = 0, out_bytes = 0;
    char *pin = nullptr, *din = nullptr, *dout = nullptr;
    hipEvent_t *ev = nullptr;  // the context's two timing events, around the launches

    explicit osg_batch_io(osg_ctx *c) : ctx(c) {}
    osg_seg in(size_t elem, size_t count) { return osg_seg_add(in_bytes, elem, count); }
    osg_seg out(size_t elem, size_t count) { return osg_seg_add(out_bytes, elem, count); }

    int stage()
    {
        pin = (char *)osg_pinned(ctx, in_bytes + out_bytes);
        if (!pin) return osg_set_error(ctx, OSG_E_NOMEM, "pinned alloc failed");
        return osg_idle(ctx);  // the pinned block may still be in use
    }
    // elements [first, first + count) of an input segment, in the pinned block
    template <class T>
    T *host_in(osg_seg s, size_t first = 0) const
    {
        return (T *)(pin + s.off + s.elem * first);
    }
    void put(osg_seg s, size_t first, const void *src, size_t count) const
    {
        if (count) std::memcpy(host_in<char>(s, first), src, s.elem * count);
    }
    int upload()
    {
        OSG_ALLOC(ctx, din, SLOT_BA0, in_bytes);
        OSG_ALLOC(ctx, dout, SLOT_BA1, out_bytes);
        return osg_upload(ctx, din, pin, in_bytes);
    }
    // called after the caller's other host work (scratch buffers, kernel attributes), so that it overlaps the upload
    int start()
    {
        ev = osg_ctx_events(ctx);
        if (!ev) return osg_set_error(ctx, OSG_E_HIP, "event create failed");
        OSG_HIP_CHECK(ctx, hipEventRecord(ev[0], ctx->stream));
        return 0;
    }
    template <class T>
    T *dev_in(osg_seg s) const
    {
        return (T *)(din + s.off);
    }
    template <class T>
    T *dev_out(osg_seg s) const
    {
        return (T *)(dout + s.off);
    }
    int finish(size_t dl_bytes)
    {
        OSG_HIP_CHECK(ctx, hipEventRecord(ev[1], ctx->stream));
        OSG_RC(osg_download(ctx, pin + in_bytes, dout, dl_bytes));
        OSG_RC(osg_wait(ctx));
        float kms = 0.f;
        OSG_HIP_CHECK(ctx, hipEventElapsedTime(&kms, ev[0], ev[1]));
        ctx->last_kernel_ms = kms;
        return 0;
    }
    // elements from `first` of an output segment, as downloaded
    template <class T>
    const T *result(osg_seg s, size_t first = 0) const
    {
        return (const T *)(pin + in_bytes + s.off + s.elem * first);
    }
    void get(void *dst, osg_seg s, size_t first, size_t count) const
    {
        if (count) std::memcpy(dst, result<char>(s, first), s.elem * count);
    }
};
