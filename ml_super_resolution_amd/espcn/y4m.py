"""
y4m.py -- YUV4MPEG2 ("Y4M") streams of 8-bit planar 4:2:0 frames: a text header, then per frame a `FRAME` line and the raw
planes (Y [H,W], U and V [(H + 1) // 2, (W + 1) // 2]) -- the payload EspcnModel.super_resolve_yuv420 and
frames.FrameResolver(layout='yuv420') take and give as it stands.  No codec and no library: a decoder writes such a stream
into a pipe and an encoder reads one.  The reference (espcn/espcn/experiment_test.py) reads image files only.

  read_header(fileobj) -> Header          width, height and the other tags in their order
  read_frames(fileobj, header, buffers)   generator of uint8 [frame_bytes] arrays, read into the caller's buffers if given
  Y4MWriter(fileobj, header)              writes the header line at once, then write(frame) per frame

Accepted colour tags: C420jpeg, C420mpeg2, C420paldv, C420, or none (the format's default is 4:2:0).  They differ in where
the chroma samples sit; the siting is IGNORED here -- chroma is replicated on the way in and box-averaged on the way out
-- and the tag is copied to the output.  Accepted interlace tags: Ip, I? or none.  Every other colour space (4:2:2, 4:4:4,
mono, ...), a bit depth above 8 (C420p10, ...) and interlaced streams (It, Ib, Im) are refused by a ValueError that names
the tag.  XCOLORRANGE=FULL / XCOLORRANGE=LIMITED gives the range when present (Header.full_range).

read_header(fileobj, formats=PLANAR_FORMATS) / Header(..., formats=PLANAR_FORMATS) widens the colour tags to C422, C444 and
C420p10, C422p10, C444p10, C420p12, C422p12, C444p12: planar frames whose samples above 8 bits are two bytes, little-endian,
the payload EspcnModel.super_resolve_yuv and frames.FrameResolver(layout='yuv', pixel_format=Header.pixel_format) take.  Mono,
4:1:1, 4:4:0, alpha planes, other depths (9, 14, 16) and interlaced streams stay refused by tag.
"""
import numpy as np

from .._lib import yuv420_frame_bytes, yuv_frame_bytes

MAGIC = b'YUV4MPEG2'
COLOUR_TAGS = ('C420jpeg', 'C420mpeg2', 'C420paldv', 'C420')
INTERLACE_TAGS = ('Ip', 'I?')
# the wide set, colour tag -> pixel format (a name of _lib.PIXEL_FORMATS); the four 8-bit 4:2:0 tags differ in siting alone
PLANAR_FORMATS = dict([(tag, 'yuv420p') for tag in COLOUR_TAGS] + [('C422', 'yuv422p'), ('C444', 'yuv444p')] +
                      [('C%sp%d' % (s, d), 'yuv%sp%dle' % (s, d)) for d in (10, 12) for s in ('420', '422', '444')])


class Header(object):
    """width, height and `tags`: every other header tag as text, in the stream's order (F, I, A, C, X...).  formats: None for
    8-bit 4:2:0 alone, or a mapping of the colour tags taken to pixel format names (PLANAR_FORMATS)."""

    def __init__(self, width, height, tags=(), formats=None):
        self.width, self.height, self.tags, self.formats = int(width), int(height), list(tags), formats
        self.pixel_format = 'yuv420p'                   # (the format's default: no C tag is 4:2:0)
        if self.width < 1 or self.height < 1:
            raise ValueError('Y4M header: W and H must be positive, got W%d H%d' % (self.width, self.height))
        for tag in self.tags:
            if tag[:1] == 'C' and formats is not None:
                digits = tag.partition('p')[2]
                if tag in formats:
                    self.pixel_format = formats[tag]
                elif tag.startswith('C4') and digits.isdigit():
                    raise ValueError('Y4M colour tag %s: a bit depth of %s, only 8, 10 and 12-bit samples are taken' % (tag, digits))
                else:
                    raise ValueError('Y4M colour tag %s: only planar 4:2:0, 4:2:2 and 4:4:4 are taken (%s, or no C tag)'
                                     % (tag, ', '.join(formats)))
            elif tag[:1] == 'C' and tag not in COLOUR_TAGS:
                digits = tag.partition('p')[2]
                if tag.startswith('C4') and digits.isdigit() and int(digits) > 8:
                    raise ValueError('Y4M colour tag %s: a bit depth of %s, only 8-bit samples are taken' % (tag, digits))
                raise ValueError('Y4M colour tag %s: only 4:2:0 is taken (%s, or no C tag)' % (tag, ', '.join(COLOUR_TAGS)))
            if tag[:1] == 'I' and tag not in INTERLACE_TAGS:
                raise ValueError('Y4M interlace tag %s: interlaced streams are not taken (Ip, I? or no I tag)' % tag)

    @property
    def frame_bytes(self):
        if self.pixel_format == 'yuv420p':
            return yuv420_frame_bytes(self.height, self.width)
        return yuv_frame_bytes(self.height, self.width, self.pixel_format)

    @property
    def full_range(self):
        """True / False from XCOLORRANGE=FULL / XCOLORRANGE=LIMITED, None when the stream does not say."""
        for tag in self.tags:
            if tag.upper() == 'XCOLORRANGE=FULL':
                return True
            if tag.upper() == 'XCOLORRANGE=LIMITED':
                return False
        return None

    def scaled(self, r):
        """The header of the super-resolved stream: W and H multiplied by r, every other tag copied."""
        return Header(self.width * r, self.height * r, self.tags, self.formats)

    def line(self):
        return ' '.join([MAGIC.decode(), 'W%d' % self.width, 'H%d' % self.height] + self.tags).encode('ascii') + b'\n'


def read_header(fileobj, formats=None):
    """Reads the header line of a binary stream; leaves it at the first FRAME line.  formats: as Header's."""
    line = fileobj.readline(4096)
    fields = line.rstrip(b'\n').split(b' ')
    if not line.endswith(b'\n') or fields[0] != MAGIC:
        raise ValueError('not a Y4M stream: it begins with %r' % line[:16])
    width = height = None
    tags = []
    for field in fields[1:]:
        if not field:
            continue
        tag = field.decode('ascii', 'replace')
        if tag[0] == 'W' or tag[0] == 'H':
            if not tag[1:].isdigit():
                raise ValueError('Y4M header: bad tag %s' % tag)
            if tag[0] == 'W':
                width = int(tag[1:])
            else:
                height = int(tag[1:])
        else:
            tags.append(tag)
    if width is None or height is None:
        raise ValueError('Y4M header: W and H are required, got %r' % line)
    return Header(width, height, tags, formats)


def _fill(fileobj, view):
    """Reads until `view` is full or the stream ends; the bytes read."""
    got = 0
    while got < len(view):
        n = fileobj.readinto(view[got:])
        if not n:
            break
        got += n
    return got


def read_frames(fileobj, header, buffers=None):
    """Generator over the frames that follow the header: each a uint8 array of header.frame_bytes bytes.  buffers: an iterable
    of writable contiguous uint8 arrays of that size (a ring, for instance: itertools.cycle); each payload is read straight
    into the next of them and that array is yielded, so it is the caller's to keep valid while in use.  None: a new array per
    frame.  `FRAME` lines may carry parameters; they are skipped.  A stream that ends inside a frame is refused by a
    ValueError that names the frame's index, after the frames before it were yielded."""
    size = header.frame_bytes
    ring = iter(buffers) if buffers is not None else None
    index = 0
    while True:
        line = fileobj.readline(4096)
        if not line:
            return
        if not line.endswith(b'\n') or line[:5] != b'FRAME' or line[5:6] not in (b'\n', b' '):
            raise ValueError('frame %d: a FRAME line is expected, got %r' % (index, line[:16]))
        out = next(ring) if ring is not None else np.empty((size,), dtype=np.uint8)
        if out.dtype != np.uint8 or out.shape != (size,) or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError('frame %d: the buffer must be a writable contiguous uint8 array of %d bytes' % (index, size))
        got = _fill(fileobj, memoryview(out))
        if got != size:
            raise ValueError('frame %d is short: %d of %d bytes (%d x %d, %s)' % (index, got, size, header.width, header.height,
                                                                                '4:2:0' if header.pixel_format == 'yuv420p' else header.pixel_format))
        yield out
        index += 1


class Y4MWriter(object):
    """Writes `header` at once, then one FRAME per write(): a uint8 array of header.frame_bytes bytes."""

    def __init__(self, fileobj, header):
        self.fileobj, self.header, self.frames = fileobj, header, 0
        fileobj.write(header.line())

    def write(self, frame):
        frame = np.asarray(frame)
        if frame.dtype != np.uint8 or frame.size != self.header.frame_bytes:
            raise ValueError('frame %d is %s of %d elements, the stream takes uint8 frames of %d bytes'
                             % (self.frames, frame.dtype, frame.size, self.header.frame_bytes))
        self.fileobj.write(b'FRAME\n')
        self.fileobj.write(memoryview(np.ascontiguousarray(frame).reshape(-1)))
        self.frames += 1
