"""Float32 restatement of one grid point of the loss landscape, theta = base + (dx x + dy y), in the form the reference's
``_set_parameter_offset`` was recorded to have (tests/golden/landscape.npz, ``offset_form`` = ``mul_mul_add_add``): four float32 operations,
each rounded on its own -- the two products, their sum, the sum with the base.  numpy rounds every float32 operation separately and never
contracts, so the expression below IS that form; ``fb_mt_landscape_point`` must reproduce it bit for bit."""
import numpy as np

FORM = "mul_mul_add_add"


def offset(base, dx, dy, x, y):
    """numpy float32 arrays of one shape, coordinates as float32 -> theta, float32."""
    base, dx, dy = (np.asarray(a, dtype=np.float32) for a in (base, dx, dy))
    cx, cy = np.float32(x), np.float32(y)
    px = dx * cx
    py = dy * cy
    d = px + py
    return base + d


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32), b.view(np.int32)))
