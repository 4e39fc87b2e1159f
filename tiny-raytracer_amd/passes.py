"""Names for what the passes queries return (tinyrt.h trt_passes): the slot of a path class in Scene.passes' [n, 2 B, 3] array, and the sums
a baker or a compositor wants of it.  A sample ends at a light (LIGHT), by missing everything (SKY) or by its bounce budget (SPENT, which
has no slot: Scene.passes returns its share separately); `depth` is the number of scatters before that, and depths >= B - 1 share the
last bin.  Host arithmetic only (numpy).

slot() is exact.  The sums below add slots in numpy and are NOT bit-defined: the device folds each slot in sample order, a sum of slots is
another order of the same terms."""
import numpy as np

LIGHT, SKY = "light", "sky"
KINDS = (LIGHT, SKY)


def bins_of(p):
    """B of a passes array [..., 2 B, 3]."""
    slots = np.shape(p)[-2]
    if np.shape(p)[-1] != 3 or slots not in (2, 4, 6, 8):
        raise ValueError("a passes array is [..., 2 * bins, 3] with bins 1 .. 4")
    return slots // 2


def slot(kind, depth, bins):
    """The slot of a sample that ended as `kind` (LIGHT or SKY) after `depth` scatters, with `bins` depth bins: min(depth, bins - 1) for
    LIGHT, bins + min(depth, bins - 1) for SKY."""
    if kind not in KINDS:
        raise ValueError("kind must be 'light' or 'sky'")
    if not 1 <= int(bins) <= 4:
        raise ValueError("bins must be 1 .. 4")
    if int(depth) < 0:
        raise ValueError("depth must not be negative")
    b = min(int(depth), int(bins) - 1)
    return b if kind == LIGHT else int(bins) + b


def emitters(p):
    """float32 [..., 3]: the light of every path that ended at a light, at any depth."""
    p = np.asarray(p)
    return p[..., :bins_of(p), :].sum(axis=-2)


def sky(p):
    """float32 [..., 3]: the light of every path that ended in the background, at any depth."""
    p = np.asarray(p)
    return p[..., bins_of(p):, :].sum(axis=-2)


def direct(p):
    """float32 [..., 3]: LIGHT and SKY at depth 0 - for a surfel its direct light, for a camera ray what it sees directly.  Needs
    bins >= 2: with one bin depth 0 is not kept apart."""
    p = np.asarray(p)
    bins = bins_of(p)
    if bins < 2:
        raise ValueError("direct light needs at least 2 depth bins")
    return p[..., 0, :] + p[..., bins, :]


def indirect(p):
    """float32 [..., 3]: LIGHT and SKY at every depth >= 1 - what a baker stores when direct light is computed at run time."""
    p = np.asarray(p)
    bins = bins_of(p)
    if bins < 2:
        raise ValueError("indirect light needs at least 2 depth bins")
    return p[..., 1:bins, :].sum(axis=-2) + p[..., bins + 1:, :].sum(axis=-2)
