"""tests/deflate_writer.py against zlib, without a GPU: the writer writes what it says, and every verdict of its catalogue is
zlib's -- so that a wrong expectation cannot reach tests/test_gpu_inflate_crafted.py, where the device is held to them."""
import zlib

import numpy as np
import pytest

import deflate_writer as dw

ZLIB_MESSAGES = ("invalid distance too far back", "invalid literal/lengths set", "invalid distances set", "invalid code lengths set",
                 "missing end-of-block", "invalid literal/length code", "invalid distance code", "too many length or distance symbols",
                 "invalid bit length repeat", "invalid block type", "invalid stored block lengths")


def test_bit_order_and_canonical_codes():
    w = dw.BitWriter()
    w.bits(0b101, 3)
    w.code(0b110, 3)                       # a Huffman code goes in most significant bit first
    w.bits(1, 2)
    assert w.getvalue() == bytes([0b01011101]) and w.nbits == 8
    # RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    codes = dw.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4])
    assert [codes[s] for s in range(8)] == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    assert dw.length_symbol(258) == (285, 0) and dw.length_symbol(257) == (284, 30) and dw.length_symbol(3) == (257, 0)
    assert dw.distance_symbol(32768) == (29, 8191) and dw.distance_symbol(24577) == (29, 0) and dw.distance_symbol(5) == (4, 0)
    lens = [0] * 20 + [3] * 7 + [0] * 150 + [5, 5] + [0] * 2
    assert dw.expand_items(dw.rle_items(lens)) == lens


def test_fixed_and_stored_blocks_are_what_zlib_writes():
    data = bytes(range(40, 130, 3)) + bytes([150, 200, 255])      # no repeats: zlib writes literals only, of 8 and 9 bits
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    d = dw.Deflate().fixed(final=True).literals(data).end_of_block()
    assert d.getvalue() == c.compress(data) + c.flush() and bytes(d.out) == data
    d = dw.Deflate().fixed(final=True).literals(b"hello, ").match(12, 7).end_of_block()
    assert zlib.decompress(d.getvalue(), -15) == b"hello, hello, hello" == bytes(d.out)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    assert dw.Deflate().stored(data, final=True).getvalue() == c.compress(data) + c.flush()


def test_bgzf_member_is_the_member_of_the_inflate_tests():
    from pepper_amd.bgzf import block_table
    stream, payload = dw.VALID[0].build()
    m = dw.bgzf_member(stream, payload)
    comp_off, comp_len, out_off, out_len = block_table(m + m, base=3)
    assert comp_off.tolist() == [18, len(m) + 18] and comp_len.tolist() == [len(stream)] * 2
    assert out_off.tolist() == [3, 3 + len(payload)] and out_len.tolist() == [len(payload)] * 2
    assert m[-8:-4] == zlib.crc32(payload).to_bytes(4, "little")


def test_the_catalogue_names_its_cases_once():
    names = [c.name for c in dw.VALID + dw.INVALID]
    assert len(set(names)) == len(names)
    assert len(dw.VALID) >= 30 and len(dw.INVALID) >= 40


@pytest.mark.parametrize("case", dw.VALID, ids=repr)
def test_zlib_accepts_every_valid_case(case):
    stream, payload = case.build()
    d = zlib.decompressobj(-15)
    assert d.decompress(stream) == payload
    assert d.eof and d.unused_data == b""
    assert len(payload) <= 65280 and 18 + len(stream) + 8 <= 65536


@pytest.mark.parametrize("case", dw.INVALID, ids=repr)
def test_zlib_refuses_every_invalid_case(case):
    stream, payload = case.build()
    key, out = dw.zlib_verdict(stream, payload)
    assert key != "ok"
    if case.zlib in ZLIB_MESSAGES:
        assert case.zlib in key                                   # zlib.error with these words
    else:
        assert case.zlib == key and key in ("unfinished", "long", "short", "differs")
    if key == "long":
        # more output than ISIZE: with ISIZE bytes of room, as a BGZF reader gives it, the stream does not finish
        d = zlib.decompressobj(-15)
        assert d.decompress(stream, len(payload)) == out[:len(payload)] and not d.eof
    if key in ("short", "differs"):
        # the stream itself is sound: what is wrong is in the member's trailer
        assert (len(out), zlib.crc32(out)) != (len(payload), zlib.crc32(payload))


def test_the_invalid_cases_cover_every_message():
    said = {c.zlib for c in dw.INVALID}
    assert set(ZLIB_MESSAGES) <= said
    assert {c.device for c in dw.INVALID} >= {"distance", "ISIZE", "over-subscribed", "incomplete", "end-of-block", "repeat", "HLIT",
                                               "length symbol", "no code", "beyond the block", "reserved", "LEN", "CRC32"}


def test_zlib_accepts_all_random_streams():
    members = dw.random_members()
    assert len(members) == dw.RANDOM_MEMBERS == 256
    kinds, longest_lit, longest_dist = set(), 0, 0
    for d in members:
        z = zlib.decompressobj(-15)
        assert z.decompress(d.getvalue()) == bytes(d.out)          # every stream: none skipped or filtered
        assert z.eof and z.unused_data == b""
        assert 1 <= len(d.blocks) <= 4 and len(d.out) <= dw.RANDOM_MAX_OUT
        kinds |= set(d.blocks)
        longest_lit, longest_dist = max(longest_lit, d.longest_lit), max(longest_dist, d.longest_dist)
    assert kinds == {"stored", "fixed", "dynamic"}
    assert longest_lit == 15 and longest_dist > 8
    again = dw.random_members()
    assert [d.getvalue() for d in again] == [d.getvalue() for d in members]      # seeded


@pytest.mark.parametrize("max_len", [15, 7, 5])
def test_complete_lengths_are_complete(max_len):
    rng = np.random.default_rng(3)
    for n in [2, 3, 4, 5, 19, 30, 31, 32, 100, 286, 288]:
        if n > (1 << max_len):
            with pytest.raises(ValueError):
                dw.complete_lengths(rng, n, max_len)
            continue
        for _ in range(20):
            lens = dw.complete_lengths(rng, n, max_len)
            assert len(lens) == n and min(lens) >= 1 and max(lens) <= max_len
            assert sum(1 << (max_len - l) for l in lens) == 1 << max_len          # Kraft equality
    with pytest.raises(ValueError):
        dw.complete_lengths(rng, 1)
