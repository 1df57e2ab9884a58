"""rubiksnet_amd -- MI355X-native RubiksShift operators and RubiksNet video backbone.

Public surface mirrors the reference package `rubiksnet`: `shiftlib` (RubiksShift2D,
RubiksShift3D, RubiksShiftBase + functionals), `AttentionShift`, `RubiksNetBackbone`,
`RubiksNet`.  All device work goes through librubiks_hip.so (include/rubiks_hip.h);
importing the package does not load it, calling an operator does.  `fin_status` reports an in-launch
reduction that gave up (its outputs are NaN) as a RubiksHipError; `metrics.StreamMeter` accumulates loss, top-k and per-class
accuracy on the device; `dataset` reads real video sets (list files, the reference's frame sampling) and feeds them through
the device crop / resize / flip; `jpeg` decodes baseline JPEG frames on the device, bit-exact to Pillow.
"""
from . import shiftlib  # noqa: F401
from . import augment  # noqa: F401
from . import dataset  # noqa: F401
from . import jpeg  # noqa: F401
from . import fin_status  # noqa: F401
from . import optim  # noqa: F401
from . import metrics  # noqa: F401
from .attention_shift import AttentionShift
from .backbone import RubiksNetBackbone
from .jpeg import decode_jpeg_frames, pack_jpeg_clips, parse_jpeg
from .metrics import StreamMeter
from .models import RubiksNet
from .shiftlib import RubiksShift2D, RubiksShift3D, RubiksShiftBase

__all__ = ["RubiksNet", "RubiksNetBackbone", "AttentionShift", "RubiksShift2D", "RubiksShift3D",
           "RubiksShiftBase", "shiftlib", "augment", "dataset", "fin_status", "optim", "metrics", "StreamMeter", "jpeg",
           "parse_jpeg", "pack_jpeg_clips", "decode_jpeg_frames"]
__version__ = "0.1.0"
