"""Coarse spaces shared by the GPU tests of the coarse level's side-stream path."""
import numpy as np


def ragged_basis(rl, k=5, short_sub=5, k_short=3):
    """POU-scaled cosine templates: k linearly independent vectors per subdomain, fewer on one of them"""
    from dune_ddm_amd.solver import pou_basis
    templates = {}
    for sd in rl.subs:
        ks = k_short if sd.id == short_sub else k
        i = (np.arange(sd.n) + 0.5) / sd.n
        templates[sd.id] = np.array([np.cos(m * np.pi * i) for m in range(ks)])
    return pou_basis(rl, templates)
