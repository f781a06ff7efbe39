"""
frames.py -- ESPCN on a frame sequence, bytes in and bytes out, with the upload of batch k + 1, the network on batch k and
the download of batch k - 1 in flight at once (the reference, espcn/espcn/experiment_test.py:148-184, resolves one image
per process; its paper is about video).

  frame_schedule(n_frames, batch, depth)  the ordered steps of a run, a pure function (no torch): planned first, walked
                                          by the runner -- so the ordering is checked without a GPU
  FrameResolver(model, height, width, batch=1, depth=3)   the ring of pinned / device byte buffers, three streams, events
                                          (layout='yuv420': planar 4:2:0 frames both ways, 1.5 bytes per pixel;
                                          layout='yuv', pixel_format=NAME: planar 4:2:2 / 4:4:4 / 10- and 12-bit frames)
  resolve_frames(model, frames, batch=1, depth=3)         convenience generator

A frame travels as 3 bytes per LR pixel up and 3 bytes per HR pixel down (EspcnModel.super_resolve_u8 decodes and encodes on
the device), a quarter of the float route's traffic.
"""
import functools

import numpy as np

from .._lib import yuv420_frame_bytes, yuv_format, yuv_frame_bytes

UPLOAD, COMPUTE, DOWNLOAD, YIELD = 'upload', 'compute', 'download', 'yield'


def iter_schedule(counts, depth):
    """The steps (op, slot, first_frame, count) for batches of the given frame counts, read lazily: a count is taken from
    `counts` exactly when its upload is listed, so a runner can feed it from a stream of frames whose length it does not know.

    Round i lists  upload(i), compute(i - c), download(i - c), yield(i - y)  with c = 1, y = depth - 1 (depth 1: c = y = 0,
    the serial order).  Batch k lives in slot k % depth.  The yield of batch k waits for its download on the host, and it is
    listed before upload(k + depth), the next occupant of its slot: that one host wait covers every reuse of the slot's four
    buffers (pinned and device input: read by upload(k) and compute(k); device and pinned output: written by compute and
    download of k + depth), so the streams need events only along upload -> compute -> download.  From depth 2 on, upload(k + 1)
    is listed before compute(k) and download(k); from depth 3 on, the host waits for download(k - 1) while compute(k) runs."""
    if depth < 1:
        raise ValueError('depth must be at least 1, got %r' % (depth,))
    c = 0 if depth == 1 else 1
    y = max(depth - 1, c)
    it = iter(counts)
    firsts, cnts = [], []
    ended, first, i = False, 0, 0
    while True:
        if not ended:
            n = next(it, None)
            if n is None:
                ended = True
            else:
                if n < 1:
                    raise ValueError('a batch holds at least one frame, got %r' % (n,))
                firsts.append(first)
                cnts.append(n)
                first += n
                yield (UPLOAD, i % depth, firsts[i], n)
        for op, lag in ((COMPUTE, c), (DOWNLOAD, c), (YIELD, y)):
            k = i - lag
            if 0 <= k < len(cnts):
                yield (op, k % depth, firsts[k], cnts[k])
        i += 1
        if ended and i - y >= len(cnts):
            return


def batch_counts(n_frames, batch):
    """[batch, batch, ..., the rest]: a last batch shorter than `batch` runs at its own size."""
    if n_frames < 0 or batch < 1:
        raise ValueError('n_frames >= 0 and batch >= 1, got %r and %r' % (n_frames, batch))
    return [min(batch, n_frames - f) for f in range(0, n_frames, batch)]


def frame_schedule(n_frames, batch, depth):
    """The ordered list of steps (op, slot, first_frame, count), op in upload / compute / download / yield, for n_frames
    frames in batches of `batch` through a ring of `depth` slots (iter_schedule has the order and why it is safe)."""
    return list(iter_schedule(batch_counts(n_frames, batch), depth))


class FrameResolver(object):
    """Owns what a run needs: per slot a pinned host input [batch,H,W,3], a device input, a device output [batch,rH,rW,3] and
    a pinned host output, all uint8; three streams (upload, compute, download) and the events between them.  It opens these
    three streams and no other, and sets no environment variable.  One resolve() at a time.

    layout='yuv420': a frame is a flat uint8 array of frame_bytes bytes, planar 4:2:0 as a Y4M stream carries it, in and out
    (hr_frame_bytes); the buffers are [batch, frame_bytes] and [batch, hr_frame_bytes], half the link traffic of 'rgb', and
    the compute step is EspcnModel.super_resolve_yuv420 with `matrix` and `full_range`.  The schedule, the streams and the
    refusal rules are the same for both layouts.

    layout='yuv', pixel_format=NAME (a name of _lib.PIXEL_FORMATS: 'yuv422p', 'yuv444p', 'yuv420p10le', ...): the same with frames
    of that format, bytes at every depth, and EspcnModel.super_resolve_yuv as the compute step."""

    def __init__(self, model, height, width, batch=1, depth=3, device=None, timing=False, layout='rgb', matrix='bt601', full_range=False,
                 pixel_format=None):
        if batch < 1 or depth < 1:
            raise ValueError('batch and depth must be at least 1, got %r and %r' % (batch, depth))
        if layout not in ('rgb', 'yuv420', 'yuv'):
            raise ValueError("layout must be 'rgb' or 'yuv420' (or 'yuv' with a pixel_format), got %r" % (layout,))
        if (layout == 'yuv') != (pixel_format is not None):
            raise ValueError("pixel_format goes with layout='yuv' and with no other, got layout %r and pixel_format %r" % (layout, pixel_format))
        if layout == 'yuv':
            yuv_format(pixel_format)                    # (an unknown name is refused here, by the list of names)
        if matrix not in ('bt601', 'bt709'):
            raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
        if int(height) < 1 or int(width) < 1:
            raise ValueError('height and width must be at least 1, got %r and %r' % (height, width))
        self.model, self.height, self.width, self.batch, self.depth = model, int(height), int(width), int(batch), int(depth)
        self.layout, self.matrix, self.full_range, self.pixel_format = layout, matrix, bool(full_range), pixel_format
        r = model.scaling_factor
        # the one place that knows the layout: a frame's shapes and byte counts, and the compute step _compute(dev_in, out=dev_out)
        if layout == 'yuv420':
            # a frame is the Y4M payload: Y [H,W], then U and V [(H + 1) // 2, (W + 1) // 2] -- 1.5 bytes per pixel each way
            self.frame_bytes = yuv420_frame_bytes(self.height, self.width)
            self.hr_frame_bytes = yuv420_frame_bytes(self.height * r, self.width * r)
            self.frame_shape, self.hr_frame_shape = (self.frame_bytes,), (self.hr_frame_bytes,)
            self._compute = functools.partial(model.super_resolve_yuv420, height=self.height, width=self.width,
                                              matrix=self.matrix, full_range=self.full_range)
        elif layout == 'yuv':
            # the same payload in any planar format of _lib.PIXEL_FORMATS: bytes at every depth, sized by the library
            self.frame_bytes = yuv_frame_bytes(self.height, self.width, pixel_format)
            self.hr_frame_bytes = yuv_frame_bytes(self.height * r, self.width * r, pixel_format)
            self.frame_shape, self.hr_frame_shape = (self.frame_bytes,), (self.hr_frame_bytes,)
            self._compute = functools.partial(model.super_resolve_yuv, height=self.height, width=self.width, pixel_format=pixel_format,
                                              matrix=self.matrix, full_range=self.full_range)
        else:
            self.frame_shape, self.hr_frame_shape = (self.height, self.width, 3), (self.height * r, self.width * r, 3)
            self.frame_bytes, self.hr_frame_bytes = self.height * self.width * 3, self.height * r * self.width * r * 3
            self._compute = model.super_resolve_u8
        import torch
        self.device = torch.device(device) if device is not None else model.stack.device
        lr, hr = (self.batch,) + self.frame_shape, (self.batch,) + self.hr_frame_shape
        self.host_in = [torch.empty(lr, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self.host_out = [torch.empty(hr, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self.dev_in = [torch.empty(lr, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        self.dev_out = [torch.empty(hr, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        self._np_in = [t.numpy() for t in self.host_in]
        self._np_out = [t.numpy() for t in self.host_out]
        self.streams = {op: torch.cuda.Stream(device=self.device) for op in (UPLOAD, COMPUTE, DOWNLOAD)}
        # timing: a start event per step as well, and stream_ms sums each stream's busy time (a measurement aid)
        self.timing = bool(timing)
        self._done = {op: [torch.cuda.Event(enable_timing=self.timing) for _ in range(self.depth)] for op in self.streams}
        self._start = {op: [torch.cuda.Event(enable_timing=True) for _ in range(self.depth)] for op in self.streams} if self.timing else None
        self.stream_ms = {op: 0.0 for op in self.streams}

    def _check(self, index, frame):
        frame = np.asarray(frame)
        if frame.dtype != np.uint8 or frame.shape != self.frame_shape:
            raise ValueError('frame %d is %s %s, this resolver takes uint8 %s'
                             % (index, frame.dtype, tuple(frame.shape), self.frame_shape))
        return frame

    def resolve(self, frames, copy=True):
        """Generator over an iterable of [H,W,3] uint8 arrays: yields (index, hr_u8 [rH,rW,3]) in input order (layout
        'yuv420' and 'yuv': [frame_bytes] uint8 arrays in, [hr_frame_bytes] out).

        copy=False yields views of the pinned output ring instead of copies.  A view stays valid until depth - 1 further
        frames have been yielded (the next download into its slot is enqueued when the generator is resumed after that);
        with depth 1, until the generator is resumed.  Use it, or copy it, before then.

        A frame of another shape or dtype is refused by a ValueError that names its index, before anything is enqueued for
        it: no further frame is read, the frames before it are resolved and yielded, and then the error is raised.  However the
        generator ends (exhausted, closed early, or by an error), it first waits for the three streams: nothing of it is left
        running."""
        import torch
        it = iter(frames)
        waiting = []                    # the frames of the batch whose upload step comes next
        state = {'index': 0, 'error': None}

        def counts():
            while state['error'] is None:
                got = []
                for frame in it:
                    try:
                        got.append(self._check(state['index'], frame))
                    except ValueError as e:
                        state['error'] = e
                        break
                    state['index'] += 1
                    if len(got) == self.batch:
                        break
                if not got:
                    return
                waiting.append(got)
                yield len(got)

        dev, st, done, start = self.device, self.streams, self._done, self._start
        for s in st.values():
            s.wait_stream(torch.cuda.current_stream(dev))       # (weights written on the caller's stream)
        try:
            for op, slot, first, n in iter_schedule(counts(), self.depth):
                if op == YIELD:
                    done[DOWNLOAD][slot].synchronize()
                    if self.timing:
                        for o in st:
                            self.stream_ms[o] += start[o][slot].elapsed_time(done[o][slot])
                    for j in range(n):
                        out = self._np_out[slot][j]
                        yield first + j, (out.copy() if copy else out)
                    continue
                with torch.cuda.stream(st[op]):
                    if op == UPLOAD:
                        for j, frame in enumerate(waiting.pop(0)):
                            self._np_in[slot][j] = frame
                    elif op == COMPUTE:
                        st[op].wait_event(done[UPLOAD][slot])
                    else:
                        st[op].wait_event(done[COMPUTE][slot])
                    if self.timing:
                        start[op][slot].record(st[op])
                    if op == UPLOAD:
                        self.dev_in[slot][:n].copy_(self.host_in[slot][:n], non_blocking=True)
                    elif op == COMPUTE:
                        self._compute(self.dev_in[slot][:n], out=self.dev_out[slot][:n])
                    else:
                        self.host_out[slot][:n].copy_(self.dev_out[slot][:n], non_blocking=True)
                    done[op][slot].record(st[op])
            if state['error'] is not None:
                raise state['error']
        finally:
            for s in st.values():
                s.synchronize()


def resolve_frames(model, frames, batch=1, depth=3, copy=True):
    """resolve() on a resolver sized by the first frame: yields (index, hr_u8) in input order."""
    it = iter(frames)
    head = next(it, None)
    if head is None:
        return
    head = np.asarray(head)
    if head.ndim != 3 or head.shape[2] != 3:
        raise ValueError('frame 0 is %s, an [H,W,3] image is expected' % (tuple(head.shape),))

    def chain():
        yield head
        for frame in it:
            yield frame

    resolver = FrameResolver(model, head.shape[0], head.shape[1], batch=batch, depth=depth)
    for item in resolver.resolve(chain(), copy=copy):
        yield item
