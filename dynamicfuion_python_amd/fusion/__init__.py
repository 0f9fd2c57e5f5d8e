"""DynamicFusion loop over this package's GPU components (reference apps/fusion/)."""
from .pipeline import (AnchorComputationMode, FusionParameters, FusionPipeline, FrameResult, GraphGenerationMode,  # noqa: F401
                       MeshExtractionWeightThresholdingMode, TrackingMethod, TrackingSpanMode)
