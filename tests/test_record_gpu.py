"""The life cycle of an IF record at the seams of the file -> HBM pipeline (csrc/sgx_record.cpp): four ring slots of
16 MiB, a synchronous upload (sgx_if_upload_file) and a background one (sgx_if_open_file), the watermark a reader
waits on, a free in mid-stream, and the allocation a freed record parks for the next one."""
import os

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

SLOT = 16 << 20
SIZE = 5 * SLOT + 12345


@pytest.fixture(scope="module")
def record_file(tmp_path_factory):
    """(path, bytes) of one file of five slots and a bit, written once."""
    data = np.random.default_rng(20).integers(-128, 128, size=SIZE, dtype=np.int8)
    path = str(tmp_path_factory.mktemp("record") / "if.bin")
    data.tofile(path)
    return path, data


def _ctx():
    m = pkg()
    return m, m.engine.get_context(m.Settings(), 0)


def _open(ctx, entry, path, off, n):
    rec = getattr(ctx, entry)(path, off, n)
    if entry == "open_file":
        rec.wait()
    return rec


# (offset, n, expected length): one byte, around one slot, all four slots from an unaligned offset, the first reuse of
# a ring slot, the whole file, a window the file ends in, a window behind its end
WINDOWS = [(0, 0, 0), (0, 1, 1), (0, SLOT - 1, SLOT - 1), (0, SLOT, SLOT), (0, SLOT + 1, SLOT + 1),
           (777, 4 * SLOT, 4 * SLOT), (0, 4 * SLOT + 1, 4 * SLOT + 1), (0, SIZE, SIZE), (SIZE - 1000, 5000, 1000),
           (SIZE + 10, 100, 0)]


@pytest.mark.parametrize("entry", ["upload_file", "open_file"])
def test_windows_at_the_slot_seams(record_file, entry):
    path, data = record_file
    m, ctx = _ctx()
    for off, n, want_len in WINDOWS:
        rec = _open(ctx, entry, path, off, n)
        try:
            assert len(rec) == want_len, (off, n)
            assert np.array_equal(rec.download(), data[off:off + n]), (off, n)
        finally:
            rec.free()


def test_prefix_wait_then_the_rest(record_file):
    path, data = record_file
    m, ctx = _ctx()
    rec = ctx.open_file(path, 0, SIZE)
    try:
        rec.wait(1)
        assert np.array_equal(rec.download(0, 1), data[:1])
        rec.wait()
        assert len(rec) == SIZE
        assert np.array_equal(rec.download(), data)
    finally:
        rec.free()


def test_free_while_streaming_leaves_the_context_usable(record_file):
    path, data = record_file
    m, ctx = _ctx()
    ctx.open_file(path, 0, SIZE).free()
    small = data[:4096]
    rec = ctx.upload(small)
    try:
        assert np.array_equal(rec.download(), small)
    finally:
        rec.free()


def _spare_sequence(ctx, path, data):
    for n in (2 * SLOT, SLOT + 5, 3 * SLOT):
        rec = ctx.upload_file(path, 0, n)
        try:
            assert len(rec) == n
            assert np.array_equal(rec.download(), data[:n]), n
        finally:
            rec.free()


def test_parked_allocation_on_and_off(record_file):
    """A freed record's allocation is parked for the next one (SLOT + 5 fits the 2 SLOT one, 3 SLOT does not), or, with
    SGX_IF_SPARE=0, given back at once: the records read the same either way."""
    path, data = record_file
    m, ctx = _ctx()
    _spare_sequence(ctx, path, data)
    old = os.environ.get("SGX_IF_SPARE")
    os.environ["SGX_IF_SPARE"] = "0"
    try:
        _spare_sequence(ctx, path, data)
    finally:
        if old is None:
            del os.environ["SGX_IF_SPARE"]
        else:
            os.environ["SGX_IF_SPARE"] = old


@pytest.mark.parametrize("entry", ["upload_file", "open_file"])
def test_missing_file_is_refused(entry):
    m, ctx = _ctx()
    with pytest.raises(m._native.SgxError) as e:
        getattr(ctx, entry)("/nonexistent/record.bin", 0, 10)
    assert str(e.value).split(": ", 1)[1].startswith("cannot open")
