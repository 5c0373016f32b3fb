from .unet import UNet  # noqa: F401
from .vae import GeneralVAESeg, GeneralVAEImage, DiagonalGaussianDistribution  # noqa: F401
from .clip_vision import CLIPVisionDescriptor  # noqa: F401
from .clip_text import CLIPTextEncoder, strip_text_prefix  # noqa: F401
