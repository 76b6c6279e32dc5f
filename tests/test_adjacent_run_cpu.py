"""adjacent_run -- the one statement of "adjacent intervals of one contig, ascending" both image drivers group by -- against the
two loops it replaced, restated literally: the variant driver's (slack 2 * REGION_SAFE_BASES) and the polish driver's (slack 1)."""
import numpy as np
import pytest

from pepper_amd.variant.PEPPER_VARIANT import adjacent_run

SAFE = 100                  # (ConsensCandidateFinder.REGION_SAFE_BASES)


def variant_loop(intervals, g0, batch, safe):
    g1 = g0 + 1
    while (g1 < len(intervals) and g1 - g0 < batch and intervals[g1][0] == intervals[g0][0]
           and intervals[g1 - 1][1] <= intervals[g1][1] <= intervals[g1 - 1][2] + 2 * safe
           and intervals[g1][2] >= intervals[g1 - 1][2]):
        g1 += 1
    return g1


def polish_loop(intervals, counter, batch):
    chr_name = intervals[counter][0]
    g1 = counter + 1
    while (g1 < len(intervals) and g1 - counter < batch and intervals[g1][0] == chr_name
           and intervals[g1 - 1][1] <= intervals[g1][1] <= intervals[g1 - 1][2] + 1
           and intervals[g1][2] >= intervals[g1 - 1][2]):
        g1 += 1
    return g1


def grid(contig, start, n, size, step=None):
    step = size if step is None else step
    return [(contig, start + k * step, start + k * step + size) for k in range(n)]


def hand_built():
    """name -> intervals; with each the run lengths from interval 0 the two slacks must give at a batch of 8."""
    a = grid("a", 0, 3, 1000)
    return {
        "abutting": (grid("a", 0, 5, 1000), 5, 5),
        "contig change": (grid("a", 0, 2, 1000) + grid("b", 2000, 3, 1000), 2, 2),
        "the same coordinates on another contig": (grid("a", 0, 2, 1000) + [("b", 2000, 3000)], 2, 2),
        "gap of the polish slack": (a + [("a", 3001, 4000)], 4, 4),
        "gap one past the polish slack": (a + [("a", 3002, 4000)], 4, 3),
        "gap of the variant slack": (a + [("a", 3000 + 2 * SAFE, 4000)], 4, 3),
        "gap one past the variant slack": (a + [("a", 3001 + 2 * SAFE, 4000)], 3, 3),
        "overlapping polish intervals": (grid("a", 0, 6, 1200, 1000), 6, 6),
        "a descending start": (a + [("a", 1999, 4000)], 3, 3),
        "the same start again": (a + [("a", 2000, 3000)], 4, 4),
        "an end that moves backwards": (a + [("a", 2500, 2999)], 3, 3),
        "batch reached in mid-run": (grid("a", 0, 12, 1000), 8, 8),
        "one interval": (grid("a", 0, 1, 1000), 1, 1),
        "a worker's next run of intervals": (grid("a", 0, 4, 1000) + grid("a", 16000, 4, 1000), 4, 4),
    }


@pytest.mark.parametrize("name", sorted(hand_built()))
def test_hand_built_lists(name):
    intervals, want_variant, want_polish = hand_built()[name]
    assert adjacent_run(intervals, 0, 8, 2 * SAFE) == variant_loop(intervals, 0, 8, SAFE) == want_variant
    assert adjacent_run(intervals, 0, 8, 1) == polish_loop(intervals, 0, 8) == want_polish
    for g0 in range(len(intervals)):
        for batch in (1, 2, 3, 8, 100):
            assert adjacent_run(intervals, g0, batch, 2 * SAFE) == variant_loop(intervals, g0, batch, SAFE), (g0, batch)
            assert adjacent_run(intervals, g0, batch, 1) == polish_loop(intervals, g0, batch), (g0, batch)


def test_seeded_lists():
    """Random walks over two contigs whose steps fall on and around every edge of the condition."""
    rng = np.random.default_rng(20261018)
    gaps = [-1200, -1, 0, 1, 2, 2 * SAFE - 1, 2 * SAFE, 2 * SAFE + 1, 5000]
    runs = set()
    for _ in range(200):
        intervals, contig, start, end = [], "a", 0, 1000
        for _ in range(int(rng.integers(1, 60))):
            intervals.append((contig, start, end))
            if rng.random() < 0.04:
                contig = "b" if contig == "a" else "a"
            start = max(0, end + int(rng.choice(gaps)) if rng.random() < 0.15 else end)
            end = start + int(rng.choice([1000, 1000, 1000, 1000, 1200, 1, 0])) if rng.random() < 0.97 else end - 1
        for g0 in range(len(intervals)):
            for batch in (1, 4, 16, 1024):
                v, p = variant_loop(intervals, g0, batch, SAFE), polish_loop(intervals, g0, batch)
                assert adjacent_run(intervals, g0, batch, 2 * SAFE) == v and adjacent_run(intervals, g0, batch, 1) == p
                runs.add((v - g0, p - g0))
    # (the lists do tell the two slacks apart, and reach runs cut by the batch)
    assert any(v > p for v, p in runs) and (16, 16) in runs and (1, 1) in runs
