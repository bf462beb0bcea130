#!/usr/bin/env python3
"""
The quintessence field behind a thawing dark-energy posterior: bands of V(phi) and a(t), and the age of the universe.

The reference's field.py reconstructs phi(a), V(phi), t(a) and a(t) for the one (H0, Om, w0) its author typed in from a fit.
Here a synthetic thawing chain (Gaussian around that triple, w0 kept above -1) is drawn on the device and
``quintessence.bands`` reconstructs the field of EVERY sample -- 5000 nodes, one workgroup per sample -- and reduces V(phi),
a(t) and t_today to their 16 / 50 / 84 % envelopes where the chain is.  The arrays go to an .npz; nothing is plotted.

    python examples/quintessence_band.py [--samples 20000] [--out quintessence_band.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--out", default="quintessence_band.npz")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    amd = importlib.import_module("cosmology-model-fit_amd")
    Q = amd.quintessence
    gen = torch.Generator(device=dev).manual_seed(11)
    centre = torch.tensor([66.53, 0.312, -0.763], dtype=torch.float64, device=dev)  # field.py:8-11
    sigma = torch.tensor([0.6, 0.008, 0.06], dtype=torch.float64, device=dev)
    samples = centre + sigma * torch.randn((args.samples, 3), dtype=torch.float64, device=dev, generator=gen)
    samples[:, 2].clamp_(min=-0.999)

    model = Q.Model(fde="thawing", columns={"H0": 0, "Om": 1, "w0": 2})
    best = Q.reconstruct(model, centre[None], phi=2000, t=1000)  # the script's own curves
    phi = best["phi_grid"][0].cpu().numpy()
    t = best["t_grid"][0].cpu().numpy()
    v_band = Q.bands(model, samples, "V_phi", phi)
    a_band = Q.bands(model, samples, "a_t", t)
    age = Q.bands(model, samples, "t_today")
    np.savez(args.out, phi=phi, V_bands=v_band["bands"], V_mean=v_band["mean"], V_best=best["V_phi"][0].cpu().numpy(),
             t=t, a_bands=a_band["bands"], a_mean=a_band["mean"], a_best=best["a_t"][0].cpu().numpy(),
             q=age["q"], age_bands=age["bands"][:, 0], age_mean=age["mean"][0], age_std=age["std"][0],
             n_used=age["n_used"], n_phantom=age["n_phantom"], n_invalid=age["n_invalid"])
    lo, med, hi = age["bands"][:, 0]
    print(f"{age['n_used']} of {args.samples} samples have a field ({age['n_phantom']} phantom, {age['n_invalid']} invalid)")
    print(f"age of the universe: {med:.3f} +{hi - med:.3f} -{med - lo:.3f} Gyr   (field.py's triple: {float(best['t_today'][0]):.3f})")
    for i in (500, 1000, 1999):
        l, m, h = v_band["bands"][:, i]
        print(f"  phi = {phi[i]:.5f}: V = {m:.4f} +{h - m:.4f} -{m - l:.4f}")
    print(f"saved phi, V_bands [3, 2000], t, a_bands [3, 1000], age_bands to {args.out}")


if __name__ == "__main__":
    main()
