"""The host side of the device stitch (pepper_amd/polish/DeviceStitch.py): plan() against what create_consensus_sequence hands to
small_chunk_stitch, the new polish() arguments, the PEPPER_AMD_DEVICE_STITCH switch and the pa_stitcher_* bindings.  No GPU."""
import inspect

import numpy as np
import pytest

from pepper_amd import _lib
from pepper_amd.polish import Stitch


class _InlinePool(object):
    """Stands in for the process pool of create_consensus_sequence: runs every submitted call at once, in this process."""

    def __init__(self, max_workers=None):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *args):
        return False

    def submit(self, fn, *args):
        value = fn(*args)

        class _Done(object):
            def result(self):
                return value
        return _Done()


def _recorded_groups(monkeypatch, keys, threads):
    """The groups create_consensus_sequence gives to small_chunk_stitch, in the order it makes them."""
    groups = []

    def record(contig, small_chunk_keys):
        groups.append(list(small_chunk_keys))
        return -1, -1, ''
    monkeypatch.setattr(Stitch, "small_chunk_stitch", record)
    monkeypatch.setattr(Stitch.concurrent.futures, "ProcessPoolExecutor", _InlinePool)
    assert Stitch.create_consensus_sequence("ctg", keys, threads) == ''
    return groups


def _keys(rng, n):
    """n regions as perform_stitch collects them: two files, a file's regions sorted by name; unsorted starts, some (start, end)
    twice (once per file)."""
    starts = rng.permutation(n) * 700
    per_file = {"a.hdf": [], "b.hdf": []}
    for k, start in enumerate(starts.tolist()):
        end = start + int(rng.integers(500, 1500))
        per_file["a.hdf" if k % 3 else "b.hdf"].append(("ctg-%d-%d" % (start, end), start, end))
        if k % 5 == 0:
            per_file["a.hdf" if not k % 3 else "b.hdf"].append(("ctg-%d-%d" % (start, end), start, end))
    keys = []
    for name in ("a.hdf", "b.hdf"):
        keys.extend((name, region, start, end) for region, start, end in sorted(per_file[name]))
    return keys[:n] if len(keys) > n else keys


@pytest.mark.parametrize("threads", [1, 2, 3, 7])
def test_plan_reproduces_the_groups_of_create_consensus_sequence(monkeypatch, threads):
    from pepper_amd.polish.DeviceStitch import plan
    rng = np.random.default_rng(100 + threads)
    for n in range(1, 41):
        keys = _keys(rng, n)
        groups = _recorded_groups(monkeypatch, keys, threads)
        p = plan(keys, threads)
        assert p.n_pieces == len(groups)
        mine = [[] for _ in range(p.n_pieces)]
        for i in p.order:
            mine[p.piece[i]].append((keys[i][0], "ctg", keys[i][2], keys[i][3]))
        assert mine == groups, (n, threads)
        assert sorted(p.rank) == list(range(len(keys))) and [p.rank[i] for i in p.order] == list(range(len(keys)))


def test_plan_threads_one_matches_the_patched_call(monkeypatch):
    """With threads = 1 the groups are the ones the patched small_chunk_stitch itself received."""
    from pepper_amd.polish.DeviceStitch import plan
    keys = _keys(np.random.default_rng(7), 11)
    groups = _recorded_groups(monkeypatch, keys, 1)
    p = plan(keys, 1)
    assert len(groups) == 1 and [(keys[i][0], "ctg", keys[i][2], keys[i][3]) for i in p.order] == groups[0]


def test_plan_keeps_file_order_for_one_region_in_two_files():
    from pepper_amd.polish.DeviceStitch import plan
    keys = [("p0.hdf", "ctg-2400-3300", 2400, 3300), ("p0.hdf", "ctg-3000-4000", 3000, 4000),
            ("p1.hdf", "ctg-0-2500", 0, 2500), ("p1.hdf", "ctg-3000-4000", 3000, 4000)]
    p = plan(keys, 1)
    assert p.order == [2, 0, 1, 3]                            # (3000, 4000): p0's before p1's
    assert p.piece == [0, 0, 0, 0] and p.n_pieces == 1
    p = plan(keys, 3)                                         # pieces of max(2, int(4 / 3) + 1) = 2 regions
    assert p.piece == [0, 1, 0, 1] and p.n_pieces == 2


def test_plan_ranks_twelve_chunks_in_string_order():
    from pepper_amd.polish.DeviceStitch import plan, string_order, string_order_key
    p = plan([("f", "ctg-0-900", 0, 900)], 1, chunk_ids=[list(range(12))])
    by_place = sorted(range(12), key=lambda c: p.chunk_order[0][c])
    assert [str(c) for c in by_place] == ["0", "1", "10", "11", "2", "3", "4", "5", "6", "7", "8", "9"]
    assert string_order(["0", "1", "10", "2"]) == [0, 1, 2, 3] and string_order([2, 10, 1]) == [2, 1, 0]
    # the key a streaming caller uses (it does not know how many chunks a region will have) orders the same way
    ids = list(range(0, 1300, 7)) + [10 ** 17, 99]
    assert sorted(ids, key=string_order_key) == sorted(ids, key=str)
    assert max(string_order_key(c) for c in ids) < 2 ** 63
    with pytest.raises(ValueError):
        string_order_key(-1)


def test_polish_takes_the_new_arguments():
    from pepper_amd.polish.polish import polish
    params = inspect.signature(polish).parameters
    assert params["device_stitch"].default is None and params["keep_predictions"].default is None
    from pepper_amd.polish.fused import FusedConsensus
    assert {"device_stitch", "keep_predictions"} <= set(inspect.signature(FusedConsensus.__init__).parameters)


def test_switch_follows_the_variable(monkeypatch):
    monkeypatch.delenv("PEPPER_AMD_DEVICE_STITCH", raising=False)
    assert _lib.device_stitch() is False
    monkeypatch.setenv("PEPPER_AMD_DEVICE_STITCH", "1")
    assert _lib.device_stitch() is True
    monkeypatch.setenv("PEPPER_AMD_DEVICE_STITCH", "0")
    assert _lib.device_stitch() is False
    assert _lib.DEVICE_STITCH_ENV == "PEPPER_AMD_DEVICE_STITCH"


def test_stitcher_entry_points_are_bound():
    names = {name for name, _, _ in _lib.SYMBOLS}
    assert {"pa_stitcher_create", "pa_stitcher_destroy", "pa_stitcher_add", "pa_stitcher_finish", "pa_stitcher_take",
            "pa_stitcher_stats", "pa_stitcher_limits"} <= names


def test_limits_and_loud_failure_without_a_device():
    """The limits need no device; a handle does, and says so (PA_ERR_NO_DEVICE) where there is none."""
    import torch
    from pepper_amd import build
    from pepper_amd.polish.DeviceStitch import DeviceStitcher
    build.build()
    lim = DeviceStitcher.limits()
    assert lim["max_position"] == 2 ** 32 - 1 and lim["max_index"] == 2 ** 16 - 1
    assert lim["scan_block"] >= 64 and lim["slab_rows"] >= 1000
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PepperAmdError, match="no CPU fallback"):
            DeviceStitcher(0)
