"""Test-side restatement of pytorch_msssim 1.0.0 `ms_ssim` (the reference's dependency, not installed here: PARITY
UNPINNED -- restated from its published algorithm, as crdr_oracle restates compressai).  Plain torch on the CPU,
parameterised by dtype: float32 is what the reference computes, float64 is the yardstick the GPU is gated against."""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN_SIZE, WIN_SIGMA = 11, 1.5


def window(dtype=torch.float32) -> torch.Tensor:
    """_fspecial_gauss_1d: built in fp32, then cast (win.to(X.dtype))."""
    coords = torch.arange(WIN_SIZE, dtype=torch.float) - WIN_SIZE // 2
    g = torch.exp(-(coords ** 2) / (2 * WIN_SIGMA ** 2))
    g /= g.sum()
    return g.to(dtype)


def gaussian_filter(x: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    """valid separable correlation, H then W, grouped per channel"""
    c = x.shape[1]
    x = F.conv2d(x, win.reshape(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(x, win.reshape(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)


def ssim(x, y, win, data_range):
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = gaussian_filter(x, win), gaussian_filter(y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11 = gaussian_filter(x * x, win) - mu1_sq
    s22 = gaussian_filter(y * y, win) - mu2_sq
    s12 = gaussian_filter(x * y, win) - mu1_mu2
    cs_map = (2 * s12 + c2) / (s11 + s22 + c2)
    ssim_map = ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
    return torch.flatten(ssim_map, 2).mean(-1), torch.flatten(cs_map, 2).mean(-1)


def pool(x: torch.Tensor) -> torch.Tensor:
    return F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 255, dtype=torch.float32) -> torch.Tensor:
    """size_average=True; gradients flow through autograd when x / y require them"""
    x, y = x.to(dtype), y.to(dtype)
    assert min(x.shape[-2:]) > (WIN_SIZE - 1) * 2 ** 4, "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % (
        (WIN_SIZE - 1) * 2 ** 4)
    win = window(dtype).to(x.device)
    weights = torch.tensor(WEIGHTS, dtype=torch.float32).to(x.device, dtype)
    mcs = []
    for i in range(len(WEIGHTS)):
        s, cs = ssim(x, y, win, data_range)
        if i < len(WEIGHTS) - 1:
            mcs.append(torch.relu(cs))
            x, y = pool(x), pool(y)
    vals = torch.stack(mcs + [torch.relu(s)], dim=0)
    return torch.prod(vals ** weights.view(-1, 1, 1), dim=0).mean()


def quantize(real: torch.Tensor, fake: torch.Tensor):
    """calc_ms_ssim's input handling: (x + 1) / 2 * 255 when real.max() <= 1, then .int().float()"""
    if real.max() <= 1.0:
        real, fake = (real + 1.) / 2. * 255., (fake + 1.) / 2. * 255.
    return real.int().float(), fake.int().float()
