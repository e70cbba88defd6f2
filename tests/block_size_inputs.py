"""Input builders of the block-size fixtures (tests/golden/block_sizes.json, tools/gen_block_size_golden.py).

The kinds of tests/golden_inputs.py plus two of their own:
  phantom_noise  a seeded phantom with seeded uniform noise of +-amp, kept in [0, 2047] (every slice round-trips, Q7);
                 optionally cropped to "shape".  Noise makes blocks difficult at every block size, so meshing happens.
  q4_run         a flat image without traversal whose block 0 (the first bs raster pixels) alternates 900 / 1100: a
                 difficult block 0, which meshes with the first candidate whatever it holds (Q4); the lower half is noise.
"""
import numpy as np

import golden_inputs as gi


def build_input(spec):
    kind = spec["kind"]
    if kind == "phantom_noise":
        img = gi.ct_phantom(spec["seed"], spec["n"]).astype(np.int32)
        rng = np.random.default_rng(spec["seed"] + 1000)
        img += rng.integers(-spec["amp"], spec["amp"] + 1, size=img.shape)
        img = np.clip(img, 0, 2047).astype(np.uint16)
        if "shape" in spec:
            w, h = spec["shape"]
            img = np.ascontiguousarray(img[:w, :h])
        return img
    if kind == "q4_run":
        w, h = spec["shape"]
        img = np.full((w, h), 1000, dtype=np.uint16)
        img.flat[: spec["bs"]] = np.where(np.arange(spec["bs"]) % 2 == 0, 900, 1100)
        rng = np.random.default_rng(spec["seed"])
        img[w // 2:, :] = rng.integers(0, 2048, size=(w - w // 2, h))
        return img
    return gi.build_input(spec)
