"""``EnhanceNetSmallDiscriminator`` (``SuperresolutionNetwork/losses/enhancenetsmall.py``): per halving one stride-1 and one stride-2
convolution (``:21-25``); at 128 x 128 ten convolutions, 16 .. 256 channels."""
from .makelayers import HalvingDiscriminator


class EnhanceNetSmallDiscriminator(HalvingDiscriminator):
    @staticmethod
    def block(channels):
        return [channels, (channels, 2)]
