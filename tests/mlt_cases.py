"""The Metropolis parity cases shared by tests/test_mlt.py (CPU) and tests/test_gpu_mlt.py: name ->
(bling_amd.scene configuration, overrides)."""

# chains 1 / 64 / 65 / 257; M not divisible by C, and M < C so that some chains do nothing; bootstrap 1,
# 100 and more than one wave of bootstrap samples; plarge 0, 0.25, 1; maxDepth 1, 5, 16; images 8 x 8 and 33 x 17
SIZES = {
    "one-chain": ("C1", "image=8,8;metropolis=1,4,100,0,1"),             # M 256: the reference's structure
    "dark-start": ("C1", "image=8,8;metropolis=1,4,1,0,1"),              # the one bootstrap sample is black: a = 0 / 0
    "wave": ("C1", "image=8,8;metropolis=5,2,100,0.25,64"),              # M 128 = 2 x 64
    "idle-chains": ("C1", "image=33,17;metropolis=5,0.1,100,1,65"),      # M 56 < 65: chains 56 .. 64 do nothing
    "ragged": ("C1", "image=33,17;metropolis=16,1,100,0.25,257"),        # M 561 = 2 x 257 + 47
    "boot-one": ("C1", "image=8,8;metropolis=5,3,1,0.25,65"),            # M 192 = 2 x 65 + 62, one bootstrap sample
    "boot-chunks": ("C1", "image=8,8;metropolis=1,1,20000,0.25,4"),      # bootstrap in two waves (16 384 + 3 616)
}
SCENES = {k: (k, None) for k in ("M1", "M2", "M3", "M4", "M5")}           # bling_amd.scene.MLT_SCENES
CASES = {**SIZES, **SCENES}


def bound(ref):
    """1.01 (n + 2) 2^-24 A64 per pixel and channel of the restatement's last pass."""
    import numpy as np
    return 1.01 * (np.repeat(ref.count.astype(np.float64), 3) + 2) * 2.0 ** -24 * ref.abs64


def ratio(err, bnd):
    import numpy as np
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bnd == 0, np.finfo(np.float64).tiny, bnd))))
