"""Stage-1 model: ELIC transforms + Minnen20 hyperprior + Charm context model
(src/models/comp_model/hyperprior_model.py:21-264 and hyperprior_charm_model.py:20-147, merged: the plain
hyperprior variants without Charm subclass this one and put an adapter in the Charm's place, hyperprior_model.py)."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import pandas as pd
import torch
from torch import Tensor

from crdr_amd.models.subnet import build_subnet
from crdr_amd.models.subnet.entropy_model.gaussian_conditional import get_scale_table
from crdr_amd.utils.codec_utils import HeaderHandler
from crdr_amd.utils.registry import MODEL_REGISTRY

from .base_model import BaseModel


@MODEL_REGISTRY.register()
class HyperpriorCharmModel(BaseModel):
    def _build_subnets(self):
        sn = self.opt.subnet
        self.encoder = build_subnet(sn.encoder, "encoder")
        self.decoder = build_subnet(sn.decoder, "decoder")
        self.hyperencoder = build_subnet(sn.hyperencoder, "hyperencoder")
        self.hyperdecoder = build_subnet(sn.hyperdecoder, "hyperdecoder")
        self.entropy_model_z = build_subnet(sn.entropy_model_z, "entropy_model")
        self.entropy_model_y = build_subnet(sn.entropy_model_y, "entropy_model")
        self.context_model = build_subnet(sn.context_model, "context_model")
        self.return_likelihoods = bool(self.opt.get("return_likelihoods", False))

    # ---- hooks the rate/beta-conditioned subclasses override
    def _encode(self, x, **cond):
        return self.encoder(x)

    def _decode(self, y_hat, **cond):
        return self.decoder(y_hat)

    def _extra_outputs(self, **cond) -> Dict:
        return {}

    # ---- staged backward (data-parallel training): with `backward_cuts` set to a dict, a training forward detaches the graph
    # at the Charm's inputs and output -- name -> (tensor upstream of the cut, leaf downstream of it; same storage) -- so the
    # trainer can run the backward in three pieces in gradient order (synthesis transform | context model | hyper-prior +
    # analysis transform) and start the all-reduce of each piece's gradients while the next piece computes
    backward_cuts: Optional[Dict[str, Tuple[Tensor, Tensor]]] = None

    def _cut(self, name: str, t: Tensor, is_train: bool) -> Tensor:
        cuts = self.backward_cuts
        if cuts is None or not is_train or not torch.is_grad_enabled() or not t.requires_grad:
            return t
        leaf = t.detach().requires_grad_(True)
        cuts[name] = (t, leaf)
        return leaf

    # ---- training / evaluation forward
    def run_model(self, real_images, is_train: bool = True, noise: Optional[Dict[str, Tensor]] = None, **cond):
        N, _, H, W = real_images.size()
        x = self.data_preprocess(real_images, is_train=is_train)
        out = self.forward(x, is_train=is_train, noise=noise, **cond)
        rate = self.get_rate_summary_dict(out, H * W)
        real, fake = self.data_postprocess(x, out["fake_images"], size=(H, W), is_train=is_train)
        return dict(real_images=real, fake_images=fake, y_hat=out["quantized_code"]["y"], z_hat=out["quantized_code"]["z"],
                    **self._extra_outputs(**cond), **rate, **out.get("others", {}))

    @torch.no_grad()
    def reconstruct(self, real_images, **cond) -> Dict[str, Tensor]:
        """Training-mode reconstruction WITHOUT the rate terms: same x̂, y_hat, z_hat as run_model(is_train=True) (STE
        rounding does not depend on the noise draws or on the scale branch), minus the scale transforms of the Charm, the
        scale branch of the hyper-decoder and every likelihood.  Used for the no-grad high-rate pass of stage 3
        (multirate_hr_rgan_beta_cond_rate_distortion_trainer.py:42-47 only keeps `fake_images` of that pass)."""
        N, _, H, W = real_images.size()
        x = self.data_preprocess(real_images, is_train=True)
        y = self._encode(x, **cond)
        z = self.hyperencoder(y)
        z_hat = self.entropy_model_z(z, is_train=True, want_bits=True)[0]
        y_hat = self.context_model.reconstruct_latent(y, self.hyperdecoder.hd_mu(z_hat), self.entropy_model_y)
        fake = self._decode(y_hat, **cond)
        real, fake = self.data_postprocess(x, fake, size=(H, W), is_train=True)
        return dict(real_images=real, fake_images=fake, y_hat=y_hat, z_hat=z_hat)

    def get_rate_summary_dict(self, out_dict: Dict, num_pixel: int) -> Dict[str, Tensor]:
        """bpp[n] = (bits_y[n] + bits_z[n]) / (H*W): noisy (`bpp`) and quantised (`qbpp`) (hyperprior_model.py:60-85).
        The bit sums come straight out of the fused entropy kernels."""
        b = out_dict["bits"]
        return dict(y_likelihood=out_dict["likelihoods"]["y"], z_likelihood=out_dict["likelihoods"]["z"],
                    bpp=(b["y"] + b["z"]) / num_pixel, bits_y=b["y"], bits_z=b["z"], num_pixel=num_pixel,
                    y_q_likelihood=out_dict["q_likelihoods"]["y"], z_q_likelihood=out_dict["q_likelihoods"]["z"],
                    qbpp=(b["y_q"] + b["z_q"]).detach() / num_pixel)

    @staticmethod
    def likelihood_to_bit(likelihood: Tensor, num_pixel: int) -> Tuple[Tensor, Tensor]:
        bit = -(torch.log(likelihood).sum(dim=tuple(range(1, likelihood.ndim)))) / np.log(2)
        return bit, bit / num_pixel

    def forward(self, real_images, is_train: bool = True, noise: Optional[Dict[str, Tensor]] = None, **cond):
        noise = noise or {}
        y = self._encode(real_images, **cond)
        z = self.hyperencoder(y)
        z_hat, z_lik, z_bits = self.entropy_model_z(z, is_train=is_train, noise=noise.get("z"), want_bits=True)
        hyper_out = self.hyperdecoder(z_hat)
        want_lik = self.return_likelihoods or not is_train
        yb: Dict = {}
        y_in, hyper_in = self._cut("y", y, is_train), self._cut("hyper_out", hyper_out, is_train)
        y_hat, y_lik, y_qlik = self.context_model(y_in, hyper_in, self.entropy_model_y, is_train=is_train,
                                                  calc_q_likelihood=True, noise=noise.get("y"), want_lik=want_lik, bits_out=yb)
        y_bits, y_qbits = yb["y"], yb["y_q"]
        fake = self._decode(self._cut("y_hat", y_hat, is_train), **cond)
        if not is_train:
            fake = torch.clamp(fake, min=-1.0, max=1.0)
        with torch.no_grad():
            if is_train:
                _, z_qlik, z_qbits = self.entropy_model_z(z.detach(), is_train=False, want_bits=True)
            else:
                z_qlik, z_qbits = z_lik, z_bits
        return {
            "fake_images": fake,
            "likelihoods": {"y": y_lik, "z": z_lik},
            "latent_code": {"y": y, "z": z},
            "quantized_code": {"y": y_hat, "z": z_hat},
            "q_likelihoods": {"y": y_qlik, "z": z_qlik},
            "bits": {"y": y_bits, "z": z_bits, "y_q": y_qbits, "z_q": z_qbits},
        }

    # ---- codec
    codec_profile: Optional[Dict[str, float]] = None  # set to {} to collect the wall-time split of compress / decompress

    def _tick(self, key: Optional[str], t0: Optional[float] = None) -> float:
        """Wall-time accounting of the codec (BASELINE config #5 reports {transforms, Charm, rANS}); active only when
        `codec_profile` is a dict -- each tick synchronises the device, so it is off in normal use."""
        import time
        if self.codec_profile is None:
            return 0.0
        torch.cuda.synchronize()
        t = time.perf_counter()
        if key is not None:
            self.codec_profile[key] = self.codec_profile.get(key, 0.0) + (t - t0)
        return t

    def _make_header_handler(self):
        return HeaderHandler(use_non_zero_ind=False)

    def codec_setup(self):
        """CDF tables for z and y.  Unlike the reference (hyperprior_model.py:126-129; hyperprior_charm_model.py:80-82)
        nothing is moved to the CPU: the HIP kernels are deterministic (fixed reduction order, no atomics), so the
        encoder and decoder sides reproduce the same mu / sigma bit for bit on the GPU; only rANS stays on the host."""
        self.header_handler = self._make_header_handler()
        self.entropy_model_z.update(force=True)
        self.entropy_model_y.update_scale_table(get_scale_table(), force=True)
        self.yC = self.encoder.latent_ch
        self.zC = self.hyperencoder.latent_ch
        self.y_stride = 2 ** self.encoder.num_downscale
        self.model_stride = self.y_stride * 2 ** self.hyperencoder.num_downscale

    def _header_encode(self, size, y_hat, **cond) -> bytes:
        return self.header_handler.encode(size, y_hat)

    def _header_cond(self, header: Dict) -> Dict:
        return {}

    # compress = compress_device (GPU: transforms, Charm, symbols / CDF indexes in coder order, asynchronous copies into
    # pinned host memory; returns without waiting) + compress_finish (host: waits for that image's copies, serial rANS,
    # header).  A sweep overlaps the two across images: while a host thread codes image k, the GPU already works on image
    # k+1 (`compress_many`; the rANS calls release the GIL).
    def _pinned(self, shape, dtype) -> Tensor:
        pool = self.__dict__.setdefault("_pin_pool", {})
        key = (tuple(shape), dtype)
        free = pool.setdefault(key, [])
        return free.pop() if free else torch.empty(shape, dtype=dtype, pin_memory=True)

    def _unpin(self, t: Tensor) -> None:
        self.__dict__.setdefault("_pin_pool", {}).setdefault((tuple(t.shape), t.dtype), []).append(t)

    @torch.no_grad()
    def compress_device(self, real_images: Tensor, **cond) -> Dict:
        N, _, H, W = real_images.shape
        assert N == 1, f"In compress mode, batchsize must be 1, but {N}"
        t = self._tick(None)
        x = self.data_preprocess(real_images, is_train=False)
        y = self._encode(x, **cond)
        z = self.hyperencoder(y)
        z_hat, z_lik = self.entropy_model_z(z, is_train=False)
        z_sym = self.entropy_model_z.quantize_symbols(z).contiguous()
        hyper_out = self.hyperdecoder(z_hat)
        t = self._tick("transforms", t)
        sym, idx, y_hat, y_lik = self.context_model.forward_compress_device(y, hyper_out, self.entropy_model_y)
        stats = torch.stack([torch.max(torch.abs(y_hat)), -torch.log2(y_lik).sum(), -torch.log2(z_lik).sum()])
        host = {"sym": self._pinned(sym.shape, torch.int32), "idx": self._pinned(idx.shape, torch.int32),
                "zsym": self._pinned(z_sym.shape, torch.int32), "stats": self._pinned((3,), torch.float32)}
        host["sym"].copy_(sym, non_blocking=True)
        host["idx"].copy_(idx, non_blocking=True)
        host["zsym"].copy_(z_sym, non_blocking=True)
        host["stats"].copy_(stats, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._tick("charm", t)
        return {"host": host, "event": ev, "size": (H, W), "cond": cond, "z_hat": z_hat, "y_hat": y_hat, "z_likelihood": z_lik,
                "y_likelihood": y_lik, "_keep": (sym, idx, z_sym, stats)}

    def compress_finish(self, ticket: Dict) -> Dict:
        import time
        from crdr_amd.codec import rans
        t0 = time.perf_counter()
        ticket["event"].synchronize()
        h = ticket["host"]
        H, W = ticket["size"]
        cdf, sizes, offs = self.entropy_model_y.host_tables()
        y_str = rans.encode_with_indexes(h["sym"].numpy().reshape(-1), h["idx"].numpy().reshape(-1), cdf, sizes, offs)
        z_str = self.entropy_model_z.compress_symbols(h["zsym"].numpy())[0]
        ymax, y_bit, z_bit = (float(v) for v in h["stats"])
        header = self._header_encode((H, W), torch.tensor([ymax]), **ticket["cond"])
        for v in h.values():
            self._unpin(v)
        if self.codec_profile is not None:
            self.codec_profile["rans"] = self.codec_profile.get("rans", 0.0) + (time.perf_counter() - t0)
        return {"string_list": [header, z_str, y_str], "z_hat": ticket["z_hat"], "y_hat": ticket["y_hat"],
                "z_likelihood": ticket["z_likelihood"], "y_likelihood": ticket["y_likelihood"], "pred_y_bit": y_bit,
                "pred_y_bpp": y_bit / (H * W), "pred_z_bit": z_bit, "pred_z_bpp": z_bit / (H * W)}

    @torch.no_grad()
    def compress(self, real_images: Tensor, **cond) -> Dict:
        return self.compress_finish(self.compress_device(real_images, **cond))

    @torch.no_grad()
    def compress_many(self, images, workers: int = 2, **cond):
        """Generator over compress() results for a sequence of [1, 3, H, W] images with the host coder of image k running
        (in `workers` threads) beside the GPU work of the following images; results come back in order."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        pending = deque()
        with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
            for img in images:
                pending.append(pool.submit(self.compress_finish, self.compress_device(img, **cond)))
                while len(pending) > workers:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()

    @torch.no_grad()
    def decompress(self, string_list: List, **cond) -> Tuple[Tensor, Tensor, Tensor]:
        assert len(string_list) == 3, f"String list length should be 3 (header, z, and y), but got {len(string_list)}"
        header = self.header_handler.decode(string_list[0])
        H, W = header["img_size"]
        s = self.model_stride
        zH, zW = int(np.ceil(H / s)), int(np.ceil(W / s))
        t = self._tick(None)
        z_symbol = self.entropy_model_z.decompress([string_list[1]], (zH, zW)).to(self.device)
        z_hat = self.entropy_model_z.dequantize(z_symbol)
        t = self._tick("rans", t)
        hyper_out = self.hyperdecoder(z_hat)
        t = self._tick("transforms", t)
        self.context_model.codec_profile = self.codec_profile
        y_hat, _ = self.context_model.forward_decompress(string_list[2], hyper_out, self.entropy_model_y)
        t = self._tick(None)
        fake = self._decode(y_hat, **self._header_cond(header), **cond)
        fake = self.data_postprocess(fake, size=(H, W), is_train=False)
        self._tick("transforms", t)
        return fake, z_hat, y_hat

    @torch.no_grad()
    def decompress_many(self, string_lists, workers: int = 2, **cond):
        """Generator over decompress() results for a sequence of [header, z, y] string lists, in order, with `workers` images in
        flight: each is decoded by its own host thread on its own HIP stream, so the serial rANS decoder of one image (C, GIL
        released) runs beside the GPU transforms of the others -- the decoder-side ping-pong of
        minnen20_charm_context_model.py:192-240 (transform a slice, decode it on the host, feed it back) no longer leaves the GPU
        idle.  Same bytes in, bit-identical y_hat / z_hat / image out as decompress() (deterministic kernels)."""
        import threading
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        local = threading.local()
        dev = torch.device(self.device)
        ready = torch.cuda.Event()
        ready.record()   # whatever prepared the model (codec_setup, weight packs) on the caller's stream

        def work(strings):
            st = getattr(local, "stream", None)
            if st is None:
                st = local.stream = torch.cuda.Stream(dev)
            with torch.no_grad(), torch.cuda.stream(st):
                st.wait_event(ready)
                out = self.decompress(strings, **cond)
                st.synchronize()
            return out
        pending = deque()
        with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
            for strings in string_lists:
                pending.append(pool.submit(work, strings))
                while len(pending) > workers:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()

    # ---- validation (bpp / PSNR / MS-SSIM over a loader)
    def _validation_conditions(self, **kw) -> List[Tuple[str, Dict]]:
        return [("", {})]

    @torch.no_grad()
    def validation(self, dataloader, max_sample_size: int, save_img: bool = False, save_dir: str = "", use_tqdm: bool = False, **kw) -> pd.DataFrame:
        from crdr_amd.utils.img_utils import calc_ms_ssim, calc_psnr, imwrite
        rows = []
        n = min(len(dataloader), max_sample_size)
        if save_img:
            assert os.path.exists(save_dir), f'save_dir: "{save_dir}" does not exist.'
        for idx, data in enumerate(dataloader):
            row = {"idx": idx + 1}
            for suffix, cond in self._validation_conditions(**kw):
                out = self.run_model(**data, is_train=False, **cond)
                row[f"bpp{suffix}"] = out["bpp"].mean().item()
                row[f"psnr{suffix}"] = calc_psnr(out["real_images"], out["fake_images"], 255)
                row[f"ms_ssim{suffix}"] = calc_ms_ssim(out["real_images"], out["fake_images"])
                if save_img:
                    imwrite(os.path.join(save_dir, f"sample_{idx + 1}_fake{suffix}.jpg"), out["fake_images"])
            rows.append(row)
            if idx + 1 == n:
                break
        return pd.json_normalize(rows)
