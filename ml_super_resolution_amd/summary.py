"""
summary.py -- TensorBoard event files without TensorFlow: what tf.summary.FileWriter writes for the reference's trainers
(scalars, image panels, the session-log START), and a reader for it.

File   <logdir>/events.out.tfevents.<10-digit unix seconds>.<hostname>, a sequence of TFRecords:
         uint64 length (LE) | uint32 mask_crc(crc32c(length bytes)) | data | uint32 mask_crc(crc32c(data))
       whose data is a serialised `Event` (tensorflow/core/util/event.proto, framework/summary.proto):
         Event          wall_time = 1 double, step = 2 int64, file_version = 3 string, summary = 5, session_log = 7
         Summary        value = 1 (repeated)
         Summary.Value  tag = 1 string, simple_value = 2 float, image = 4
         Summary.Image  height = 1, width = 2, colorspace = 3, encoded_image_string = 4 (PNG)
         SessionLog     status = 1 (START = 1)
       The first record is Event{wall_time, file_version: "brain.Event:2"}.
Writer EventFileWriter queues to ONE background thread, as TensorFlow's does: the train loop never waits for a value to
       arrive on the host, for the PNG encoder or for the disk -- only for room in the bounded queue.
Reader read_events(path) checks both CRCs of every record and yields plain dicts.

The CRC and the protobuf field encoders are tf_bundle's.  The PNG byte stream (zlib's default level, filter 0) is this
module's own: TensorFlow's differs byte for byte and decodes to the same pixels.
"""
import os
import queue
import socket
import struct
import threading
import time
import zlib

import numpy as np

from . import tf_bundle as _tb

FILE_VERSION = 'brain.Event:2'
SESSION_LOG_START = 1
_MASK64 = (1 << 64) - 1


# ---- encoding --------------------------------------------------------------------------------------------------------
def encode_png(rgb):
    """[H,W,3] uint8 -> an 8-bit RGB PNG (one IDAT, every row with filter 0)."""
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError('a panel must be a uint8 [H,W,3] array, got %s %s' % (rgb.dtype, rgb.shape))
    h, w, _ = rgb.shape
    raw = np.zeros((h, 1 + 3 * w), np.uint8)
    raw[:, 1:] = rgb.reshape(h, 3 * w)

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw.tobytes())) + chunk(b'IEND', b''))


def decode_png(data):
    """A PNG's pixels as a numpy array (Pillow)."""
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def _encode_value(tag, kind, payload):
    body = _tb.pb_bytes_field(1, tag.encode())
    if kind == 'scalar':                                        # payload: the 4 bytes of a little-endian float32
        body += _tb.put_varint((2 << 3) | 5) + payload
    else:                                                       # payload: [H,W,3] uint8
        h, w, _ = payload.shape
        image = (_tb.pb_varint_field(1, h) + _tb.pb_varint_field(2, w) + _tb.pb_varint_field(3, 3) +
                 _tb.pb_bytes_field(4, encode_png(payload)))
        body += _tb.pb_bytes_field(4, image)
    return _tb.pb_bytes_field(1, body)


def encode_event(wall_time, step=0, file_version=None, values=None, session_log=None):
    """One serialised Event.  values: [(tag, 'scalar', 4 bytes of float32) | (tag, 'image', uint8 [H,W,3])]."""
    out = _tb.pb_fixed64_field(1, struct.unpack('<Q', struct.pack('<d', wall_time))[0]) if wall_time != 0 else b''
    if step:
        out += _tb.pb_varint_field(2, int(step) & _MASK64)
    if file_version is not None:
        out += _tb.pb_bytes_field(3, file_version.encode())
    if values is not None:
        out += _tb.pb_bytes_field(5, b''.join(_encode_value(*v) for v in values))
    if session_log is not None:
        out += _tb.pb_bytes_field(7, _tb.pb_varint_field(1, int(session_log)))
    return out


def scalar_event(wall_time, step, tag, value):
    """Event{wall_time, step, summary{value{tag, simple_value}}} of one Python float."""
    return encode_event(wall_time, step, values=[(tag, 'scalar', struct.pack('<f', value))])


def _crc(data):
    data = bytes(data)
    crc = _tb.crc32c(data) if len(data) < 4096 else _tb.crc32c_array(np.frombuffer(data, np.uint8))
    return struct.pack('<I', _tb.mask_crc(crc))


def frame_record(data):
    """The TFRecord around one serialised message."""
    length = struct.pack('<Q', len(data))
    return length + _crc(length) + data + _crc(data)


# ---- reading ---------------------------------------------------------------------------------------------------------
def _decode_value(buf):
    v = {}
    for fn, wt, x in _tb.pb_fields(buf):
        if fn == 1 and wt == 2:
            v['tag'] = x.decode()
        elif fn == 2 and wt == 5:
            v['simple_value'] = struct.unpack('<f', struct.pack('<I', x))[0]
        elif fn == 4 and wt == 2:
            names = {1: 'height', 2: 'width', 3: 'colorspace', 4: 'encoded_image_string'}
            image = {'height': 0, 'width': 0, 'colorspace': 0, 'encoded_image_string': b''}
            image.update({names[f]: y for f, _, y in _tb.pb_fields(x) if f in names})
            v['image'] = image
    return v


def decode_event(data):
    """A serialised Event as a dict: wall_time, step, and file_version (str) / session_log (the status) / values (a list
    of {'tag', 'simple_value'} and {'tag', 'image': {height, width, colorspace, encoded_image_string}})."""
    ev = {'wall_time': 0.0, 'step': 0}
    for fn, wt, x in _tb.pb_fields(data):
        if fn == 1 and wt == 1:
            ev['wall_time'] = struct.unpack('<d', struct.pack('<Q', x))[0]
        elif fn == 2 and wt == 0:
            ev['step'] = x - (1 << 64) if x >> 63 else x
        elif fn == 3 and wt == 2:
            ev['file_version'] = x.decode()
        elif fn == 5 and wt == 2:
            ev['values'] = [_decode_value(y) for f, w, y in _tb.pb_fields(x) if f == 1 and w == 2]
        elif fn == 7 and wt == 2:
            ev['session_log'] = dict((f, y) for f, _, y in _tb.pb_fields(x)).get(1, 0)
    return ev


def read_records(path):
    """The data of every TFRecord of a file, in order; ValueError on a CRC mismatch or a truncated tail."""
    with open(path, 'rb') as f:
        buf = f.read()
    pos = 0
    while pos < len(buf):
        if pos + 12 > len(buf):
            raise ValueError('%s: truncated record header at byte %d' % (path, pos))
        if buf[pos + 8:pos + 12] != _crc(buf[pos:pos + 8]):
            raise ValueError('%s: length CRC mismatch at byte %d' % (path, pos))
        n = struct.unpack_from('<Q', buf, pos)[0]
        if pos + 12 + n + 4 > len(buf):
            raise ValueError('%s: record of %d bytes at byte %d is cut short' % (path, n, pos))
        data = buf[pos + 12:pos + 12 + n]
        if buf[pos + 12 + n:pos + 16 + n] != _crc(data):
            raise ValueError('%s: data CRC mismatch in the record at byte %d' % (path, pos))
        yield data
        pos += 16 + n


def read_events(path):
    """One dict per record of an event file (decode_event); ValueError on a CRC mismatch or a truncated tail."""
    for data in read_records(path):
        yield decode_event(data)


def event_files(logdir):
    """The event files of a log directory, oldest first."""
    return sorted(os.path.join(logdir, n) for n in os.listdir(logdir) if n.startswith('events.out.tfevents.'))


# ---- writing ---------------------------------------------------------------------------------------------------------
class EventFileWriter(object):
    """tf.summary.FileWriter(logdir) for scalars, image panels and the session log.

    add_summary(step, values): `values` is an ordered list of (tag, scalar) and (tag, panel); a scalar is a Python or numpy
    number or a one-element float32 tensor, a panel a uint8 [H,W,3] tensor or array.  A DEVICE tensor is copied into pinned
    host memory asynchronously on the current stream, followed by an event: add_summary returns without waiting for either
    (no .item(), no stream synchronisation), and the tensor may be overwritten by later launches on that stream.  One
    background thread waits for the event, encodes the PNG and appends the record, so records appear in the order of the
    add_* calls.  At most `max_queue` calls are pending; the next one blocks until there is room (TensorFlow's max_queue).
    An exception in the thread is raised by the next add_* / flush / close."""

    def __init__(self, logdir, max_queue=10):
        os.makedirs(logdir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(now), socket.gethostname()))
        self._file = open(self.path, 'wb')
        self._queue = queue.Queue(max(1, int(max_queue)))
        self._error = None
        self._closed = False
        self._pinned = {}                    # (dtype, shape) -> idle pinned buffers, handed back by the thread
        self._file.write(frame_record(encode_event(now, file_version=FILE_VERSION)))
        self._file.flush()
        self._thread = threading.Thread(target=self._run, name='EventFileWriter', daemon=True)
        self._thread.start()

    # -- the calling thread
    def _raise_pending(self):
        if self._error is not None:
            err, self._error = self._error, None
            raise RuntimeError('the event writer thread failed: %r' % (err,)) from err

    def _stage(self, kind, v):
        """-> (payload, None) for a host value, (pinned buffer with a copy in flight, device) for a device tensor"""
        import torch
        if isinstance(v, torch.Tensor):
            if kind == 'scalar':
                if v.numel() != 1 or v.dtype != torch.float32:
                    raise ValueError('a scalar tensor must hold one float32, got %s %s' % (v.dtype, tuple(v.shape)))
            elif v.dtype != torch.uint8 or v.dim() != 3 or v.shape[2] != 3:
                raise ValueError('a panel must be a uint8 [H,W,3] tensor, got %s %s' % (v.dtype, tuple(v.shape)))
            if v.is_cuda:
                key = (v.dtype, tuple(v.shape))
                idle = self._pinned.setdefault(key, [])
                buf = idle.pop() if idle else torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                buf.copy_(v, non_blocking=True)
                return buf, v.device
            v = v.detach().numpy().copy()
        if kind == 'scalar':
            return struct.pack('<f', float(np.asarray(v, np.float32).reshape(()))), None
        v = np.array(v, copy=True)
        if v.dtype != np.uint8 or v.ndim != 3 or v.shape[2] != 3:
            raise ValueError('a panel must be a uint8 [H,W,3] array, got %s %s' % (v.dtype, v.shape))
        return v, None

    def _put(self, item):
        if self._closed:
            raise ValueError('the event writer is closed')
        self._raise_pending()
        self._queue.put(item)

    def add_summary(self, step, values):
        import torch
        staged, events = [], {}
        for tag, v in values:
            kind = 'scalar' if (np.ndim(v) == 0 if not isinstance(v, torch.Tensor) else v.numel() == 1 and v.dim() <= 1) else 'image'
            payload, device = self._stage(kind, v)
            staged.append((tag, kind, payload, device is not None))
            if device is not None and device not in events:
                events[device] = None
        for device in events:                                    # after the last copy: one event per device that has one
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
            events[device] = ev
        self._put(('summary', time.time(), int(step), staged, list(events.values())))

    def add_session_log_start(self, step):
        self._put(('session_log', time.time(), int(step), SESSION_LOG_START, []))

    def flush(self):
        """Returns when every record added so far is in the file."""
        if not self._closed:
            self._queue.join()
            self._file.flush()
        self._raise_pending()

    def close(self):
        if not self._closed:
            self._closed = True
            self._queue.put(None)
            self._thread.join()
            self._file.close()
        self._raise_pending()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- the writer thread
    def _write(self, item):
        what, wall_time, step, payload, events = item
        if what == 'session_log':
            data = encode_event(wall_time, step, session_log=payload)
        else:
            for ev in events:
                ev.synchronize()
            values = []
            for tag, kind, p, pinned in payload:
                if pinned:
                    a = p.numpy()
                    values.append((tag, kind, a.tobytes() if kind == 'scalar' else a))
                else:
                    values.append((tag, kind, p))
            data = encode_event(wall_time, step, values=values)
            for tag, kind, p, pinned in payload:
                if pinned:
                    self._pinned[(p.dtype, tuple(p.shape))].append(p)
        self._file.write(frame_record(data))

    def _run(self):
        while True:
            item = self._queue.get()
            try:
                if item is None:
                    return
                if self._error is None:                          # after a failure: drain, so that nobody waits forever
                    self._write(item)
            except BaseException as e:                           # noqa: B902 -- handed to the calling thread
                self._error = e
            finally:
                self._queue.task_done()
