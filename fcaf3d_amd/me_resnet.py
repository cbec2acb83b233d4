"""Sparse ResNet backbone — host-side mirror of mmdet3d/models/backbones/me_resnet.py (ResNetBase :8-99,
MEResNet3D :102-123): same class names, constructor arguments, sub-module names (conv1.{0..3},
layer{1..4}.{j}.{conv1,norm1,conv2,norm2,downsample.{0,1}}) and parameter shapes, on HIP operators."""
from torch import nn

from . import nn as MEnn
from .registry import BACKBONES


class ResNetBase(nn.Module):
    BLOCK = None
    LAYERS = ()
    INIT_DIM = 64
    PLANES = (64, 128, 256, 512)

    def __init__(self, in_channels, n_outs):
        super().__init__()
        self.n_outs = n_outs
        self.inplanes = self.INIT_DIM
        # stem: conv k3 s2 -> instance norm -> ReLU -> max-pool k2 s2   (tensor stride 1 -> 2 -> 4)
        self.conv1 = nn.Sequential(
            MEnn.MinkowskiConvolution(in_channels, self.inplanes, kernel_size=3, stride=2, dimension=3),
            MEnn.MinkowskiInstanceNorm(self.inplanes),
            MEnn.MinkowskiReLU(inplace=True),
            MEnn.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3))
        for i in range(min(n_outs, 4)):
            setattr(self, f'layer{i + 1}', self._make_layer(self.BLOCK, self.PLANES[i], self.LAYERS[i], stride=2))

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, MEnn.MinkowskiConvolution):
                MEnn.kaiming_normal_(m.kernel, mode='fan_out', nonlinearity='relu')
            if isinstance(m, MEnn.MinkowskiBatchNorm):
                nn.init.constant_(m.bn.weight, 1)
                nn.init.constant_(m.bn.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1, dilation=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                MEnn.MinkowskiConvolution(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride,
                                          dimension=3),
                MEnn.MinkowskiBatchNorm(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride=stride, dilation=dilation, downsample=downsample, dimension=3)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, stride=1, dilation=dilation, dimension=3))
        return nn.Sequential(*layers)

    def forward(self, x):
        outs = []
        x = MEnn.run_sequential(self.conv1, x)
        for i in range(min(self.n_outs, 4)):
            x = getattr(self, f'layer{i + 1}')(x)
            outs.append(x)
        return outs


@BACKBONES.register_module()
class MEResNet3D(ResNetBase):
    _ARCH = {14: (MEnn.BasicBlock, (1, 1, 1, 1)), 18: (MEnn.BasicBlock, (2, 2, 2, 2)),
             34: (MEnn.BasicBlock, (3, 4, 6, 3)), 50: (MEnn.Bottleneck, (4, 3, 6, 3)),
             101: (MEnn.Bottleneck, (3, 4, 23, 3))}

    def __init__(self, in_channels, depth, n_outs=4, frozen_stages=-1, norm_eval=False):
        """frozen_stages (optional; the reference's config dicts build unchanged): mmdet's ResNet._freeze_stages / train(), third
        party and not in the reference tree, restated for this backbone:

          -1      nothing is frozen (the default: today's model, same parameters, names and state dict)
           0      the stem: conv1.0's kernel and conv1.1's instance-norm weight and bias get requires_grad=False (an instance norm
                  has no running statistics: its forward is unchanged)
          k >= 1  additionally layer1 .. layerk: their parameters get requires_grad=False and the modules are KEPT in eval() by
                  `train(mode)`, so their MinkowskiBatchNorm use the running statistics and do not update them

        Values outside -1 .. min(n_outs, 4) raise ValueError.

        norm_eval (mmdet's switch of the same name; a bool, anything else raises ValueError): after `train(True)` EVERY MinkowskiBatchNorm of
        the backbone is in eval() — it normalises with its running statistics and leaves them alone — while the convolutions, gamma and
        beta outside the frozen prefix keep training (the backward through such a layer: csrc/norm_eval.h).  Parameters, their names and
        the state dict are unchanged.

        What the native executor compiles: every combination of the two arguments with BasicBlock depths (executor.freeze_plan); flags
        set by hand that no declaration implies, and the Bottleneck depths, train on the module path."""
        if depth not in self._ARCH:
            raise ValueError(f'invalid depth={depth}')
        self.BLOCK, self.LAYERS = self._ARCH[depth]
        super().__init__(in_channels, n_outs)
        if not isinstance(frozen_stages, int) or not -1 <= frozen_stages <= min(n_outs, 4):
            raise ValueError(f'invalid frozen_stages={frozen_stages!r}: -1 .. {min(n_outs, 4)}')
        if not isinstance(norm_eval, bool):
            raise ValueError(f'invalid norm_eval={norm_eval!r}: a bool')
        self.frozen_stages, self.norm_eval = frozen_stages, norm_eval
        self._freeze_stages()

    def frozen_modules(self):
        """the stem and the levels that `frozen_stages` freezes, in forward order"""
        if self.frozen_stages < 0:
            return []
        return [self.conv1] + [getattr(self, f'layer{i}') for i in range(1, self.frozen_stages + 1)]

    def _freeze_stages(self):
        for m in self.frozen_modules():
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, MEnn.MinkowskiBatchNorm):
                    m.eval()
        return self
