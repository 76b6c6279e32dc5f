"""The device inflate (csrc/inflate.hip) on hand-built DEFLATE streams: tests/deflate_writer.py's catalogue and its random
streams, whose verdicts tests/test_deflate_writer_cpu.py pins to zlib.  What zlib accepts the device returns bit for bit; what
zlib refuses fails the call naming the member -- and leaves the members beside it alone: a wavefront's checks are what keeps it
inside its own slot of a buffer it shares with every other member of the call."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_writer as dw
from pepper_amd import _lib
from pepper_amd.bgzf import DeviceInflater, block_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "PEPPER_AMD_CRAFTED_FORMS_CHILD"


def _members(cases):
    built = [c.build() for c in cases]
    return [dw.bgzf_member(s, p) for s, p in built], [p for _, p in built]


def _inflate_and_compare(inf, members, expect, names):
    buf = b"".join(members)
    table = block_table(buf)
    assert len(table[0]) == len(members)
    got = inf.inflate(buf, table).tobytes()
    at = 0
    for name, want in zip(names, expect):                          # (member by member: a failure names its case)
        assert got[at:at + len(want)] == want, name
        at += len(want)
    assert at == len(got)


def test_valid_catalogue():
    members, expect = _members(dw.VALID)
    names = [c.name for c in dw.VALID]
    with DeviceInflater() as inf:
        _inflate_and_compare(inf, members, expect, names)
        # once more in reverse order: every member's output offset has another alignment
        _inflate_and_compare(inf, members[::-1], expect[::-1], names[::-1])


def test_random_streams():
    streams = [d.getvalue() for d in dw.random_members()]
    expect = [zlib.decompress(s, -15) for s in streams]            # what zlib decodes is the payload
    assert len(streams) == 256 and max(len(e) for e in expect) <= 4096
    members = [dw.bgzf_member(s, e) for s, e in zip(streams, expect)]
    with DeviceInflater() as inf:
        _inflate_and_compare(inf, members, expect, ["random stream %d" % k for k in range(len(members))])


def _neighbours():
    rng = np.random.default_rng(31)
    out = []
    for level in (6, 1):
        data = bytes(np.clip(rng.normal(30, 8, 700), 0, 93).astype(np.uint8)) + b"ACGT" * 40
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append((dw.bgzf_member(c.compress(data) + c.flush(), data), data))
    return out


def _raw_inflate(lib, h, buf, table, out):
    comp = np.frombuffer(buf, np.uint8)
    comp_off, comp_len, out_off, out_len = table
    return lib.pa_inflater_inflate(h, comp.ctypes.data, comp.size, len(comp_off), comp_off.ctypes.data, comp_len.ctypes.data,
                                   out_off.ctypes.data, out_len.ctypes.data, out.ctypes.data, out.size, 1)


def test_invalid_catalogue():
    """One call per case, the bad member between two sound ones: never first or last in the buffers, so that a missing check
    reads and writes inside the call's own allocations.  pa_inflater_inflate copies the output back before it reports: the
    neighbours' slots must hold their payloads after every failing call."""
    (first, first_data), (last, last_data) = _neighbours()
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.pa_inflater_create(0, ctypes.byref(h)))
    try:
        failed = []
        for case in dw.INVALID:
            stream, payload = case.build()
            buf = first + dw.bgzf_member(stream, payload) + last
            table = block_table(buf)
            assert len(table[0]) == 3
            out = np.full(len(first_data) + len(payload) + len(last_data), 0x3c, np.uint8)
            rc = _raw_inflate(lib, h, buf, table, out)
            text = lib.pa_last_error().decode() if rc else "accepted"
            if rc != _lib.PA_ERR_INVALID or "BGZF block 1: " not in text or (case.device and case.device not in text):
                failed.append("%s: %s (expected %r)" % (case.name, text, case.device))
            if out[:len(first_data)].tobytes() != first_data or out[out.size - len(last_data):].tobytes() != last_data:
                failed.append("%s: a neighbour's output was overwritten" % case.name)
        assert not failed, "\n".join(failed)
        # the handle is sound afterwards
        buf = first + last
        out = np.zeros(len(first_data) + len(last_data), np.uint8)
        assert _raw_inflate(lib, h, buf, block_table(buf), out) == _lib.PA_OK
        assert out.tobytes() == first_data + last_data
    finally:
        lib.pa_inflater_destroy(h)


def test_crafted_streams_through_the_encoder_entry():
    """pa_encoder_inflate_bgzf is the image drivers' entry to the same kernel: the same bytes, the same member and reason."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.pa_encoder_create(0, None, ctypes.byref(h)))

    def call(buf, out):
        comp = np.frombuffer(buf, np.uint8)
        comp_off, comp_len, out_off, out_len = block_table(buf)
        return lib.pa_encoder_inflate_bgzf(h, comp.ctypes.data, comp.size, len(comp_off), comp_off.ctypes.data, comp_len.ctypes.data,
                                           out_off.ctypes.data, out_len.ctypes.data, out.size, out.ctypes.data)
    try:
        members, expect = _members(dw.VALID)
        want = b"".join(expect)
        out = np.zeros(len(want), np.uint8)
        _lib.check(call(b"".join(members), out))
        assert out.tobytes() == want
        (first, first_data), (last, last_data) = _neighbours()
        by_name = {c.name: c for c in dw.INVALID}
        for name, reason in (("distance = bytes produced + 1: a 3-byte match in a small step", "match distance beyond the start of the block"),
                             ("incomplete distance set of two codes", "incomplete Huffman code")):
            stream, payload = by_name[name].build()
            out = np.zeros(len(first_data) + len(payload) + len(last_data), np.uint8)
            assert call(first + dw.bgzf_member(stream, payload) + last, out) == _lib.PA_ERR_INVALID, name
            assert lib.pa_last_error().decode() == "BGZF block 1: " + reason, name
        out = np.zeros(len(first_data) + len(last_data), np.uint8)
        _lib.check(call(first + last, out))
        assert out.tobytes() == first_data + last_data
    finally:
        lib.pa_encoder_destroy(h)


@pytest.mark.skipif(os.environ.get(CHILD) == "1", reason="the child run itself")
@pytest.mark.parametrize("wide,below", [("0", "48"), ("1", "1"), ("1", "64")])
def test_every_case_in_the_other_step_forms(wide, below):
    """PA_INFLATE_WIDE / PA_INFLATE_WIDE_BELOW pin the kernel's step form for a whole process: every case of this module through
    the one-window step, through the two-window step that falls back after every step of more than a byte, and through the
    always-two-window step (as tests/test_gpu_inflate.py does for its own cases).  One child at a time."""
    env = dict(os.environ, PA_INFLATE_WIDE=wide, PA_INFLATE_WIDE_BELOW=below)
    env[CHILD] = "1"
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                          "-k", "not other_step_forms"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    assert "\n4 passed" in run.stdout, run.stdout[-500:]           # (the child ran the four tests above)
