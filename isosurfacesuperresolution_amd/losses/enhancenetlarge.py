"""``EnhanceNetLargeDiscriminator`` (``SuperresolutionNetwork/losses/enhancenetlarge.py``), the trainer's default
(``mainVideoUnshaded.py:89``): per halving two stride-1 convolutions and one of stride 2 (``:21-25``); at 128 x 128 fifteen convolutions."""
from .makelayers import HalvingDiscriminator


class EnhanceNetLargeDiscriminator(HalvingDiscriminator):
    @staticmethod
    def block(channels):
        return [channels, channels, (channels, 2)]
