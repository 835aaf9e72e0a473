"""Host-side mirrors of the reference's ``src/features`` hot-path modules."""
from .stft import MelSpectrogramExtractor
from .mel_sliding_window import MelAudioBuffer, MelSlidingWindowExtractor, create_mel_extractor

__all__ = ["MelSpectrogramExtractor", "MelAudioBuffer", "MelSlidingWindowExtractor", "create_mel_extractor"]
from .opensmile_extractor import AudioBuffer, OpenSMILEeGeMAPSExtractor, create_opensmile_extractor  # noqa: E402

__all__ += ["AudioBuffer", "OpenSMILEeGeMAPSExtractor", "create_opensmile_extractor"]
from .clip_emotion import ClipEmotion  # noqa: E402

__all__ += ["ClipEmotion"]
from .basic_emotion import BasicEmotion  # noqa: E402

__all__ += ["BasicEmotion"]
from .resample import Resampler, StreamPlan, resample_filter, resample_ratio  # noqa: E402

__all__ += ["Resampler", "StreamPlan", "resample_filter", "resample_ratio"]
