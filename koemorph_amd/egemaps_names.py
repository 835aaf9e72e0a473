"""Names of the 88 eGeMAPSv02 functionals in openSMILE's output order (what `smile.feature_names` lists for
FeatureSet.eGeMAPSv02 / FeatureLevel.Functionals); km_egemaps_functionals writes its outputs in this order."""
from typing import List

FEATURE_NAMES: List[str] = (
    [f"F0semitoneFrom27.5Hz_sma3nz_{s}" for s in ("amean", "stddevNorm", "percentile20.0", "percentile50.0", "percentile80.0",
                                                   "pctlrange0-2", "meanRisingSlope", "stddevRisingSlope", "meanFallingSlope",
                                                   "stddevFallingSlope")] +
    [f"loudness_sma3_{s}" for s in ("amean", "stddevNorm", "percentile20.0", "percentile50.0", "percentile80.0", "pctlrange0-2",
                                     "meanRisingSlope", "stddevRisingSlope", "meanFallingSlope", "stddevFallingSlope")] +
    ["spectralFlux_sma3_amean", "spectralFlux_sma3_stddevNorm"] +
    [f"mfcc{i}_sma3_{s}" for i in (1, 2, 3, 4) for s in ("amean", "stddevNorm")] +
    [f"{n}_sma3nz_{s}" for n in ("jitterLocal", "shimmerLocaldB", "HNRdBACF", "logRelF0-H1-H2", "logRelF0-H1-A3",
                                  "F1frequency", "F1bandwidth", "F1amplitudeLogRelF0", "F2frequency", "F2bandwidth",
                                  "F2amplitudeLogRelF0", "F3frequency", "F3bandwidth", "F3amplitudeLogRelF0")
     for s in ("amean", "stddevNorm")] +
    [f"{n}V_sma3nz_{s}" for n in ("alphaRatio", "hammarbergIndex", "slope0-500", "slope500-1500", "spectralFlux",
                                   "mfcc1", "mfcc2", "mfcc3", "mfcc4") for s in ("amean", "stddevNorm")] +
    [f"{n}UV_sma3nz_amean" for n in ("alphaRatio", "hammarbergIndex", "slope0-500", "slope500-1500", "spectralFlux")] +
    ["loudnessPeaksPerSec", "VoicedSegmentsPerSec", "MeanVoicedSegmentLengthSec", "StddevVoicedSegmentLengthSec",
     "MeanUnvoicedSegmentLength", "StddevUnvoicedSegmentLength", "equivalentSoundLevel_dBp"])
assert len(FEATURE_NAMES) == 88

# GeMAPS v01b as it is defined here: the 88 without the spectral flux, MFCC 1-4, the bandwidths of F2 and F3 and the equivalent
# sound level, in the order the 88 have (KM_FEATURE_SET_GEMAPS writes these columns).  That openSMILE's own GeMAPSv01b has these
# values in this order is UNPINNED, as the whole back end is.
GEMAPS_REMOVED = ("spectralFlux", "mfcc", "F2bandwidth", "F3bandwidth", "equivalentSoundLevel")
GEMAPS_COLUMNS: List[int] = [i for i, n in enumerate(FEATURE_NAMES) if not any(r in n for r in GEMAPS_REMOVED)]
GEMAPS_FEATURE_NAMES: List[str] = [FEATURE_NAMES[i] for i in GEMAPS_COLUMNS]
assert len(GEMAPS_COLUMNS) == 62

# The low-level descriptors per frame (feature_level="LowLevelDescriptors"; km_egemaps_llds writes its columns in this order): the
# smoothed contours behind the functionals above.  GeMAPS: the same without the spectral flux, MFCC 1-4 and the bandwidths of F2 and
# F3.  That openSMILE's own descriptor level has these names in this order is UNPINNED, as the whole back end is.
LLD_NAMES: List[str] = (
    ["Loudness_sma3", "alphaRatio_sma3", "hammarbergIndex_sma3", "slope0-500_sma3", "slope500-1500_sma3", "spectralFlux_sma3"] +
    [f"mfcc{i}_sma3" for i in (1, 2, 3, 4)] +
    ["F0semitoneFrom27.5Hz_sma3nz", "jitterLocal_sma3nz", "shimmerLocaldB_sma3nz", "HNRdBACF_sma3nz", "logRelF0-H1-H2_sma3nz",
     "logRelF0-H1-A3_sma3nz"] +
    [f"F{i}{n}_sma3nz" for i in (1, 2, 3) for n in ("frequency", "bandwidth", "amplitudeLogRelF0")])
assert len(LLD_NAMES) == 25
GEMAPS_LLD_COLUMNS: List[int] = [i for i, n in enumerate(LLD_NAMES) if not any(r in n for r in GEMAPS_REMOVED)]
GEMAPS_LLD_NAMES: List[str] = [LLD_NAMES[i] for i in GEMAPS_LLD_COLUMNS]
assert len(GEMAPS_LLD_COLUMNS) == 18
LLD_DIMS = {"eGeMAPSv02": 25, "GeMAPS": 18}
LLD_FPS_RANGE = (1.0, 400.0)

FEATURE_SETS = {"eGeMAPSv02": 0, "GeMAPS": 1}         # the reference's spellings -> KM_FEATURE_SET_*
FEATURE_SET_DIMS = {"eGeMAPSv02": 88, "GeMAPS": 62}


def feature_set_code(feature_set: str) -> int:
    """KM_FEATURE_SET_* of a feature set's name; any other string is refused with the reference's text."""
    if feature_set not in FEATURE_SETS:
        raise ValueError(f"Unsupported feature set: {feature_set}")
    return FEATURE_SETS[feature_set]


def check_compression_shape(layer, feature_set: str = "eGeMAPSv02") -> None:
    """The compression layer of a feature set is a Linear(3 * dim, 256) -- three windows concatenated: Linear(264, 256), or
    Linear(186, 256) for GeMAPS (where the reference hard-codes 264 and so never compresses; a deliberate deviation)."""
    n_in = 3 * FEATURE_SET_DIMS[feature_set]
    if tuple(layer.weight.shape) != (256, n_in):
        raise ValueError(f"compression_layer must be a Linear({n_in}, 256), got weight {tuple(layer.weight.shape)}")


def lld_fps_value(fps) -> float:
    """The `fps` of a descriptor call as the C ABI takes it: 0.0 for None (the native 100 Hz), else a finite rate within 1 .. 400."""
    if fps is None:
        return 0.0
    fps = float(fps)
    if not (LLD_FPS_RANGE[0] <= fps <= LLD_FPS_RANGE[1]):            # NaN fails both comparisons
        raise ValueError(f"fps must be finite and within 1 .. 400, got {fps}")
    return fps


def lld_output_frames(length: int, fps: float, sample_rate: int = 16000) -> int:
    """Rows of the frame grid over `length` samples: int(L / sr * fps) in float64, in that order -- the frame count of
    MelSpectrogramExtractor.forward (reference src/features/stft.py:130)."""
    return int(length / sample_rate * lld_fps_value(fps))
