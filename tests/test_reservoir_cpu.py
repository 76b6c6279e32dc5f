"""pa_reservoir_sample (include/pepper_amd_io.h; csrc/reservoir.h, the sampler the device runs in reservoir_keep_kernel) against
the loop it restates -- pepper_amd/variant/AlignmentSummarizer.py:49-57 with numpy.random.RandomState -- slot for slot."""
import numpy as np
import pytest

SEED = 2719747673          # AlingerOptions.RANDOM_SEED of both pipelines


def _numpy_slots(seed, n, k):
    """The reference's reservoir sample on read indices, verbatim."""
    random = np.random.RandomState(seed)
    sample = []
    for i in range(n):
        if len(sample) < k:
            sample.append(i)
        else:
            j = random.randint(0, i + 1)
            if j < k:
                sample[j] = i
    return np.asarray(sample, np.int32)


def _cases():
    seen = set()
    for k in (0, 1, 2, 7, 1500, 5000):
        for n in (k, k + 1, 2 * k + 3, 20000, 70000):
            if (n, k) not in seen:
                seen.add((n, k))
                yield n, k


@pytest.mark.parametrize("n,k", list(_cases()))
def test_slots_equal_numpy(n, k):
    from pepper_amd import _lib
    got = _lib.reservoir_sample(SEED, n, k)
    want = _numpy_slots(SEED, n, k)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("rate", [0.5, 0.999])
@pytest.mark.parametrize("n", [1, 2, 3, 1001, 4999, 5000, 5001, 5006, 9999, 10001, 20000])
def test_rates_turned_into_k_by_the_python_expression(rate, n):
    """k = int(min(MAX_READS_IN_REGION, downsample_rate * total_reads)) as the variant driver's host form computes it."""
    from pepper_amd import _lib
    k = int(min(5000, rate * n))
    assert k < n
    assert np.array_equal(_lib.reservoir_sample(SEED, n, k), _numpy_slots(SEED, n, k))


def test_other_seeds_and_the_edges():
    from pepper_amd import _lib
    for seed in (0, 1, 5489, 0xffffffff):
        assert np.array_equal(_lib.reservoir_sample(seed, 3000, 40), _numpy_slots(seed, 3000, 40))
    assert len(_lib.reservoir_sample(SEED, 0, 5)) == 0
    assert np.array_equal(_lib.reservoir_sample(SEED, 4, 9), np.arange(4))          # fewer reads than slots: all of them
    with pytest.raises(ValueError):
        _lib.reservoir_sample(SEED, -1, 3)


def test_declared_bound_and_exported():
    from pepper_amd import h5
    from pepper_amd.variant import bam
    assert "pa_reservoir_sample" in {name for name, _, _ in bam.SYMBOLS}
    assert hasattr(h5.load(), "pa_reservoir_sample")
