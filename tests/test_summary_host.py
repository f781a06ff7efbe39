"""CPU-side checks of the TensorBoard summaries: the event-file writer and reader (ml_super_resolution_amd/summary.py)
against known-answer bytes and against an independent decoder (tests/summary_reference.py), and the argument checks of
the panel encoder's entry points (srx_summary_panel_u8 / _range), which refuse before any launch."""
import os
import re
import socket

import numpy as np
import pytest
import torch

from ml_super_resolution_amd import summary
from tests import summary_reference as R

EVENT_HEX = '09000000000000f83f10072a0d0a0b0a046c6f7373150000803e'


def test_known_answer_event_and_record():
    data = summary.scalar_event(1.5, 7, 'loss', 0.25)
    assert data.hex() == EVENT_HEX
    assert summary.frame_record(data).hex() == '1a00000000000000' + '129bd82d' + EVENT_HEX + 'c9d07b8d'
    # the independent message classes serialise the same event to the same bytes
    ev = R.message_class('Event')(wall_time=1.5, step=7)
    ev.summary.value.add(tag='loss', simple_value=0.25)
    assert ev.SerializeToString().hex() == EVENT_HEX
    assert summary.decode_event(data) == {'wall_time': 1.5, 'step': 7, 'values': [{'tag': 'loss', 'simple_value': 0.25}]}


def test_file_name_and_first_record(tmp_path):
    logdir = tmp_path / 'a' / 'logs'                             # created if missing
    w = summary.EventFileWriter(str(logdir))
    w.close()
    (name,) = os.listdir(str(logdir))
    assert re.match(r'^events\.out\.tfevents\.\d{10}\.' + re.escape(socket.gethostname()) + '$', name), name
    assert w.path == str(logdir / name) and summary.event_files(str(logdir)) == [w.path]
    (first,) = list(summary.read_events(w.path))
    assert first['file_version'] == 'brain.Event:2' and first['step'] == 0
    assert int(first['wall_time']) == int(name.split('.')[3])
    assert R.decode_file(w.path) == [first]


def test_scalars_panel_and_session_log_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    panel = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    panel[0, 0] = (0, 128, 255)
    with summary.EventFileWriter(str(tmp_path)) as w:
        w.add_session_log_start(40)
        w.add_summary(41, [('loss', torch.tensor(0.1, dtype=torch.float32))])                  # a 0-d tensor
        w.add_summary(42, [('loss', torch.tensor([2.5])), ('sd_sr_hd/image/0', torch.from_numpy(panel)), ('psnr', 31.25)])
        w.add_summary(43, [('patches/image', panel)])                                          # a numpy panel, alone in its event
        w.add_summary(0, [('loss', np.float32(0.0))])                                          # step 0 and value 0 are still written
        w.flush()
        assert len(list(summary.read_events(w.path))) == 6                                     # flush(): everything is in the file
    got = list(summary.read_events(w.path))
    assert got == R.decode_file(w.path)
    assert [e['step'] for e in got] == [0, 40, 41, 42, 43, 0]
    assert got[1]['session_log'] == summary.SESSION_LOG_START == 1 and 'values' not in got[1]
    assert got[2]['values'] == [{'tag': 'loss', 'simple_value': float(np.float32(0.1))}]
    assert [v['tag'] for v in got[3]['values']] == ['loss', 'sd_sr_hd/image/0', 'psnr']
    assert got[3]['values'][0]['simple_value'] == 2.5 and got[3]['values'][2]['simple_value'] == 31.25
    assert got[5]['values'] == [{'tag': 'loss', 'simple_value': 0.0}]
    for image in (got[3]['values'][1]['image'], got[4]['values'][0]['image']):
        assert (image['height'], image['width'], image['colorspace']) == (5, 7, 3)
        np.testing.assert_array_equal(R.png_pixels(image['encoded_image_string']), panel)
        np.testing.assert_array_equal(summary.decode_png(image['encoded_image_string']), panel)
    assert all(a['wall_time'] <= b['wall_time'] for a, b in zip(got, got[1:]))


def test_record_order_is_call_order_with_a_full_queue(tmp_path):
    w = summary.EventFileWriter(str(tmp_path), max_queue=4)       # 200 calls through 4 slots: add_summary blocks, nothing is lost
    for k in range(200):
        w.add_summary(k + 1, [('loss', float(k) * 0.5)])
    w.close()
    w.close()                                                     # idempotent
    got = R.decode_file(w.path)[1:]
    assert [e['step'] for e in got] == list(range(1, 201))
    assert [e['values'][0]['simple_value'] for e in got] == [k * 0.5 for k in range(200)]
    with pytest.raises(ValueError):
        w.add_summary(201, [('loss', 0.0)])                       # closed


def test_reader_refuses_damaged_files(tmp_path):
    with summary.EventFileWriter(str(tmp_path)) as w:
        w.add_summary(1, [('loss', 1.0)])
        w.add_summary(2, [('loss', 2.0)])
    good = open(w.path, 'rb').read()
    assert len(list(summary.read_events(w.path))) == 3
    first = 16 + int.from_bytes(good[:8], 'little')               # the second record starts here

    def damaged(name, data):
        p = str(tmp_path / name)
        with open(p, 'wb') as f:
            f.write(data)
        return p
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x10]) + b[i + 1:]
    for name, data in (('data_byte', flip(good, first + 12 + 3)), ('length_crc', flip(good, first + 9)),
                       ('length', flip(good, first + 1)), ('cut_mid_record', good[:len(good) - 7]),
                       ('cut_mid_header', good[:first + 5])):
        with pytest.raises(ValueError):
            list(summary.read_events(damaged(name, data)))
    assert len(list(summary.read_events(damaged('whole', good)))) == 3


def test_writer_thread_failure_surfaces_on_the_next_call(tmp_path):
    w = summary.EventFileWriter(str(tmp_path))
    real = w._file

    class Broken(object):
        def write(self, data):
            raise OSError('disk full')

        def flush(self):
            pass

        def close(self):
            real.close()
    w._file = Broken()
    w.add_summary(1, [('loss', 1.0)])
    with pytest.raises(RuntimeError, match='disk full'):
        w.flush()
    w.close()


def test_writer_refuses_malformed_values(tmp_path):
    with summary.EventFileWriter(str(tmp_path)) as w:
        with pytest.raises(ValueError):
            w.add_summary(1, [('panel', np.zeros((4, 4), np.uint8))])
        with pytest.raises(ValueError):
            w.add_summary(1, [('panel', torch.zeros((4, 4, 3), dtype=torch.float32))])
        with pytest.raises(ValueError):
            w.add_summary(1, [('loss', torch.zeros(1, dtype=torch.float64))])
    assert len(R.decode_file(w.path)) == 1


def test_panel_entry_points_refuse_bad_arguments():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    for name in ('srx_summary_panel_u8', 'srx_summary_panel_range', 'srx_summary_panel_bytes', 'srx_summary_panel_range_bytes'):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.srx_summary_panel_range_bytes() >= 8
    # never dereferenced: every case below is refused before any launch (this test runs without a GPU)
    X, OUT = 0x100000, 0x800000

    def srcs(*entries):
        arr = (_lib.PanelSrc * max(1, len(entries)))()
        for k, (x, w) in enumerate(entries):
            arr[k] = _lib.PanelSrc(x, w, 0, 0, 0)
        return arr
    two = srcs((X, 4), (X + 0x10000, 4))
    panel = 2 * 4 * 8 * 3                                          # N = 2, H = 4, widths 4 + 4, r = 1
    assert L.srx_summary_panel_bytes(two, 2, 2, 4, 1) == panel
    assert L.srx_summary_panel_bytes(srcs((X, 17), (X + 0x100000, 17)), 2, 64, 17, 3) == 64 * 17 * 3 * 34 * 3 * 3
    src_bytes = 2 * 4 * 4 * 3 * 4
    cases = [('null', (None, 2, 2, 4, 1, None, OUT)), ('null', (two, 2, 2, 4, 1, None, None)),
             ('null', (srcs((X, 4), (None, 4)), 2, 2, 4, 1, None, OUT)),
             ('r 0', (two, 2, 2, 4, 0, None, OUT)), ('r 5', (two, 2, 2, 4, 5, None, OUT)),
             ('n_src 0', (two, 0, 2, 4, 1, None, OUT)), ('n_src 9', (two, 9, 2, 4, 1, None, OUT)),
             ('bad dims', (two, 2, 0, 4, 1, None, OUT)), ('bad dims', (two, 2, 2, -1, 1, None, OUT)),
             ('bad dims', (srcs((X, 4), (X + 0x10000, 0)), 2, 2, 4, 1, None, OUT)),
             ('overlaps source 0', (two, 2, 2, 4, 1, None, X + src_bytes - 1)),        # out begins on source 0's last byte
             ('overlaps source 1', (two, 2, 2, 4, 1, None, X + 0x10000 - panel + 1)),  # out ends on source 1's first byte
             ('pitch', (srcs_pitched(_lib, X, 4, 11, 0), 1, 2, 4, 1, None, OUT))]      # a row pitch shorter than the row
    for want, args in cases:
        rc = L.srx_summary_panel_u8(*args, None)
        msg = L.srx_last_error()
        assert rc == -1 and b'summary_panel_u8' in msg and want.encode() in msg, (want, rc, msg)
    assert L.srx_summary_panel_u8(srcs((X + 2, 4)), 1, 2, 4, 1, None, OUT, None) == -5              # SRX_ERR_ALIGN
    # out just clear of both sources is not an overlap, but cannot be launched here: only the refusals are exercised
    for want, args in (('null', (two, 2, 2, 4, 1, None)), ('null', (None, 2, 2, 4, 1, OUT)), ('r 5', (two, 2, 2, 4, 5, OUT)),
                       ('n_src 0', (two, 0, 2, 4, 1, OUT)), ('overlaps source 0', (two, 2, 2, 4, 1, X + 16))):
        rc = L.srx_summary_panel_range(*args, None)
        msg = L.srx_last_error()
        assert rc == -1 and b'summary_panel_range' in msg and want.encode() in msg, (want, rc, msg)


def srcs_pitched(_lib, x, w, row_pitch, image_pitch):
    arr = (_lib.PanelSrc * 1)()
    arr[0] = _lib.PanelSrc(x, w, 0, row_pitch, image_pitch)
    return arr
