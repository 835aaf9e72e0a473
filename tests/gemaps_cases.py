"""Shared by the GeMAPS tests (tests/test_gemaps_host.py, tests/test_gpu_gemaps.py, tests/test_gpu_emotion_gemaps.py,
tests/test_gpu_train_gemaps.py): the column list written out, the compression layer of a GeMAPS object and its TWIN.

The oracle for everything behind the functionals is an eGeMAPS object with a padded layer: ``scatter_compression(L186)`` is the
``Linear(264, 256)`` whose columns ``GEMAPS_COLUMNS + 88 w`` (w = 0, 1, 2) hold L186's weights and whose other 78 columns are 0.0.
Both objects sum a row as ONE sequential fmaf chain over k from +0; ``fmaf(0, x, acc) == acc`` for the finite x the scrub
guarantees (a product of 0 and a finite x is +-0, and acc + +-0 is acc: acc starts at +0 and a sum that is exactly zero rounds to +0),
so the chain of the twin goes through the GeMAPS object's 186 partial sums in its order: EQUAL EMOTION BITS.  L186 is drawn from a
seeded normal, so that no bias is +-0 (the last step is ``acc + bias``)."""
import functools

import numpy as np
import torch

from koemorph_amd.egemaps_names import GEMAPS_COLUMNS

# the removed indices as the definition lists them: spectral flux and MFCC 1-4 over all frames (20-29), the bandwidths of F2 (48, 49)
# and F3 (54, 55), flux and MFCC 1-4 over voiced frames (66-75), the flux over unvoiced frames (80), the equivalent sound level (87)
REMOVED = tuple(range(20, 30)) + (48, 49, 54, 55) + tuple(range(66, 76)) + (80, 87)
COLUMNS = tuple(i for i in range(88) if i not in REMOVED)
COLS = np.asarray(GEMAPS_COLUMNS)
FLUX_MFCC_FIELDS = slice(5, 10)            # R_FLUX, R_MFCC .. R_MFCC + 3 of a frame record: 0 in a GeMAPS call's records


@functools.lru_cache(maxsize=None)
def l186(seed: int = 186) -> torch.nn.Linear:
    layer = torch.nn.Linear(186, 256)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(256, 186, generator=g) * 0.05)
        layer.bias.copy_(torch.randn(256, generator=g) * 0.05)
    assert bool((layer.bias != 0).all()) and bool((layer.weight != 0).all())
    return layer


def scatter_compression(layer186: torch.nn.Linear) -> torch.nn.Linear:
    """The twin's Linear(264, 256): L186's weights in the kept columns of each of the three windows, 0.0 elsewhere; L186's bias."""
    assert tuple(layer186.weight.shape) == (256, 186)
    twin = torch.nn.Linear(264, 256)
    with torch.no_grad():
        twin.weight.zero_()
        for w in range(3):
            twin.weight[:, COLS + 88 * w] = layer186.weight[:, 62 * w:62 * (w + 1)]
        twin.bias.copy_(layer186.bias)
    return twin


def bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(a, b) -> bool:
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))
