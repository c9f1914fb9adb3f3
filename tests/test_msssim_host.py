"""MS-SSIM / L1 distortion losses: what holds without a GPU -- the losses build from their YAML form, and the test-side
restatement of pytorch_msssim (tests/msssim_ref.py) behaves as the published algorithm says."""
import pytest
import torch

from tests import msssim_ref as R


@pytest.mark.parametrize("name", ["MSSSIMLoss", "L1Loss"])
def test_distortion_losses_build(name):
    from crdr_amd.losses import build_loss
    loss = build_loss({"type": name, "loss_weight": 1.0}, loss_name="distortion_loss")
    assert type(loss).__name__ == name
    assert (loss.lamb_msssim if name == "MSSSIMLoss" else loss.lamb_l1) == 1.0


def test_restatement_identity_and_window():
    g = R.window()
    assert g.shape == (11,) and abs(g.sum().item() - 1.0) < 1e-6
    assert torch.equal(g, g.flip(0))
    x = torch.rand(2, 3, 170, 180, generator=torch.Generator().manual_seed(0)) * 2 - 1
    assert abs(R.ms_ssim(x, x, 1.0, torch.float64).item() - 1.0) < 1e-12
    assert abs(R.ms_ssim(x, x, 1.0).item() - 1.0) < 1e-5


def test_restatement_size_assertion():
    x = torch.zeros(1, 3, 160, 200)
    with pytest.raises(AssertionError):
        R.ms_ssim(x, x, 1.0)
    x = torch.rand(1, 3, 161, 161, generator=torch.Generator().manual_seed(1))
    v = R.ms_ssim(x, x * 0.9, 1.0)
    assert 0 < v.item() < 1


def test_restatement_pooled_sizes():
    # odd side 2k + 1 -> k + 1 (padding side % 2, count_include_pad), even 2k -> k
    sizes, h, w = [], 197, 263
    x = torch.zeros(1, 1, h, w)
    for _ in range(4):
        x = R.pool(x)
        sizes.append(tuple(x.shape[2:]))
    assert sizes == [(99, 132), (50, 66), (25, 33), (13, 17)]
    y = R.pool(torch.ones(1, 1, 3, 3))
    assert y.shape[2:] == (2, 2) and y[0, 0, 0, 0].item() == 0.25 and y[0, 0, 1, 1].item() == 1.0
