"""The oracle (oracle/models_np.py, oracle/torch_port.py) against the golden vectors that
tests/golden/make_golden.py produced from the REFERENCE model classes.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import models_np, torch_port
from pepper_amd import synthetic

TOL = 2e-6   # fp32 restatement vs ATen: accumulation-order noise only


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


@pytest.mark.parametrize("tag", ["g1", "g3"])
def test_variant_numpy_oracle_matches_reference(golden_dir, tag):
    g = _load(golden_dir, f"variant_{tag}.npz")
    sd = synthetic.variant_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
    probs, inter = models_np.variant_forward(sd, g["images"], return_intermediates=True)
    assert np.abs(inter["enc"][:2] - g["enc2"]).max() < TOL
    assert np.abs(inter["dec"][:2] - g["dec2"]).max() < TOL
    assert np.abs(inter["logits"] - g["logits"]).max() < 2e-5 * max(1.0, np.abs(g["logits"]).max())
    assert np.abs(probs - g["probs"]).max() < 1e-5
    assert (probs.argmax(1) == g["probs"].argmax(1)).all()


def test_variant_two_layer(golden_dir):
    g = _load(golden_dir, "variant_l2.npz")
    sd = synthetic.variant_state_dict(seed=int(g["seed"]), gain=float(g["gain"]), gru_layers=2)
    probs = models_np.variant_forward(sd, g["images"], gru_layers=2)
    assert np.abs(probs - g["probs"]).max() < 1e-5


@pytest.mark.parametrize("tag", ["g1", "g3"])
def test_variant_torch_port_matches_reference(golden_dir, tag):
    g = _load(golden_dir, f"variant_{tag}.npz")
    sd = synthetic.variant_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
    model = torch_port.load_numpy_state_dict(torch_port.VariantPort(), sd)
    with torch.no_grad():
        probs = model(torch.from_numpy(g["images"]).float()).numpy()
        probs64 = model.double()(torch.from_numpy(g["images"]).double()).numpy()
    # the same model as the reference classes: their float64 forward, reproduced whatever CPU runs the test (~1e-14 apart)
    assert np.abs(probs64 - g["probs64"]).max() < 1e-10
    # float32, the reference's own dtype: exact on the CPU the vectors were made on, a few 1e-6 apart on another thread count
    # or vector width at gain 3
    assert np.abs(probs - g["probs"]).max() < 1e-5


@pytest.mark.parametrize("tag", ["g1", "g3"])
def test_polish_numpy_oracle_matches_reference(golden_dir, tag):
    g = _load(golden_dir, f"polish_{tag}.npz")
    sd = synthetic.polish_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
    labels, phred, inter = models_np.polish_predict_chunks(sd, g["images"], 128,
                                                            return_intermediates=True)
    assert np.abs(inter["hiddens"] - g["hiddens"]).max() < 2e-5
    assert np.abs(inter["acc"] - g["acc"]).max() < 2e-5
    # labels/phred are discontinuous in acc: allow flips only where the reference itself is
    # within float noise of a tie / an integer phred boundary
    top2 = np.sort(g["acc"], axis=2)[:, :, -2:]
    tie = (top2[:, :, 1] - top2[:, :, 0]) < 1e-4
    assert ((labels == g["labels"]) | tie).all()
    frac = g["phred_f32"] - np.floor(g["phred_f32"])
    near_int = (frac < 1e-3) | (frac > 1 - 1e-3)
    assert ((phred == g["phred"]) | near_int | tie).all()
    assert (labels == g["labels"]).mean() > 0.999


@pytest.mark.parametrize("tag", ["g1", "g3"])
def test_polish_torch_port_matches_reference(golden_dir, tag):
    g = _load(golden_dir, f"polish_{tag}.npz")
    sd = synthetic.polish_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
    model = torch_port.load_numpy_state_dict(torch_port.PolishPort(), sd)
    labels, phred = torch_port.polish_predict_chunks(model, g["images"], 128)
    assert (labels == g["labels"]).all()
    assert (phred == g["phred"]).all()


def test_synthetic_inputs_are_deterministic():
    a = synthetic.variant_windows(8)
    b = synthetic.variant_windows(8)
    assert a.dtype == np.int8 and a.shape == (8, 33, 26) and (a == b).all()
    p = synthetic.polish_chunks(2)
    assert p.dtype == np.uint8 and p.shape == (2, 1000, 10)
    assert p.astype(int).sum(axis=2).max() <= 254


def test_polish_two_layer_oracle(golden_dir):
    g = _load(golden_dir, "polish_l2.npz")
    sd = synthetic.polish_state_dict(seed=int(g["seed"]), gain=float(g["gain"]), gru_layers=2)
    logits, hidden = models_np.polish_forward(sd, g["x"], g["hidden"], gru_layers=2)
    assert np.abs(logits - g["logits"]).max() < 2e-5 * max(1.0, np.abs(g["logits"]).max())
    assert np.abs(hidden - g["hidden_out"]).max() < 2e-5
