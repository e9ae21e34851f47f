from .imaug import datatransform, imspec_augmentor, seg_augmentor  # noqa: F401

__all__ = ["datatransform", "seg_augmentor", "imspec_augmentor"]
