"""MI355X-native implementation of the DRAM DC3D forward/backward hot path.

Host side of libdram_hip.so: ctypes binding (`_lib`), autograd Functions
(`functional`), nn.Module leaves (`modules`) and the device optimisers (`optim`).  The drop-in modules that mirror
the reference's flat `parts.py` / `models.py` live one directory up.
"""
from . import _lib, functional, modules, optim  # noqa: F401
from .optim import SGD, AdaBound, Adam, AdamW, RAdam  # noqa: F401

# the augmentation transforms of `augment`, importable from here; the module is loaded on first use
_AUGMENT = ("GaussianBlur", "RandomMaskOut", "RandomFlip", "RandomRotate90", "GaussianAddictive", "IntensityInverse",
            "GammaTransform", "ContrastStretchingTransform", "ContrastJitter", "MinimalIntensityProjection",
            "MaximumIntensityProjection", "MinimalIntensityAxialProjection", "DiskMaskOut", "RandomCubeMask", "RandomMoveAxis",
            "RandomRotateInplane90", "RandomCrop", "StandarizeChannel", "RandomAffineTransform3D", "RandomRotate",
            "EnsembleScanAugmentation")

# the segmentation losses of `losses`, the same way
_LOSSES = ("BootBinCrossEntropy", "BinaryCrossEntropySmooth", "TverskyLoss", "SoftDiceLoss", "FocalLoss")

# the lesion-wise report of `lesions`, the same way
_LESIONS = ("label_components", "component_stats", "remove_small", "lobe_burden", "lesion_report")

# the lesion density report of `density`, the same way
_DENSITY = ("label_density", "hist_summary", "label_report")

# the lesion distribution report of `distribution`, the same way
_DISTRIBUTION = ("lung_depth", "label_depth", "lesion_distribution")

# the lesion shape report of `shape`, the same way
_SHAPE = ("label_shape", "crossings", "euler_number", "crofton_weights", "lesion_shape")

# the lesion texture report of `texture`, the same way
_TEXTURE = ("label_glcm", "glcm_features", "lesion_texture")

# the heat-map evaluation curves of `curves`, the same way
_CURVES = ("score_tables", "curves_from_tables", "heatmap_curves")

# the surface-distance metrics of `surface`, the same way
_SURFACE = ("distance_transform", "mask_surface", "surface_distances")

# the pseudo-vessel mask of `vessels`, the same way
_VESSELS = ("gaussian_derivative_taps", "hessian", "vesselness", "vessel_mask", "pseudo_vessel_mask")

# the edge-aware heat-map refinement of `refine`, the same way
_REFINE = ("guided_filter", "refine_heatmap")

# the result contact sheet of `sheet`, the same way
_SHEET = ("sheet_layout", "pick_slices", "sheet_occupancy", "result_sheet", "save_sheet")

# the views of test-time augmentation at inference (`inference`), the same way
_INFERENCE = ("tta_views",)

__all__ = ["_lib", "functional", "modules", "optim", "Adam", "AdamW", "SGD", "RAdam", "AdaBound", *_AUGMENT, *_LOSSES, *_LESIONS,
           *_DENSITY, *_DISTRIBUTION, *_SHAPE, *_TEXTURE, *_CURVES, *_SURFACE, *_VESSELS, *_REFINE, *_SHEET, *_INFERENCE]


def __getattr__(name):
    if name in _AUGMENT:
        from . import augment
        return getattr(augment, name)
    if name in _LOSSES:
        from . import losses
        return getattr(losses, name)
    if name in _LESIONS:
        from . import lesions
        return getattr(lesions, name)
    if name in _DENSITY:
        from . import density
        return getattr(density, name)
    if name in _DISTRIBUTION:
        from . import distribution
        return getattr(distribution, name)
    if name in _SHAPE:
        from . import shape
        return getattr(shape, name)
    if name in _TEXTURE:
        from . import texture
        return getattr(texture, name)
    if name in _CURVES:
        from . import curves
        return getattr(curves, name)
    if name in _SURFACE:
        from . import surface
        return getattr(surface, name)
    if name in _VESSELS:
        from . import vessels
        return getattr(vessels, name)
    if name in _REFINE:
        from . import refine
        return getattr(refine, name)
    if name in _SHEET:
        from . import sheet
        return getattr(sheet, name)
    if name in _INFERENCE:
        from . import inference
        return getattr(inference, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
