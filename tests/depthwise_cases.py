"""Geometries of the depthwise kernels' tests (csrc/dwconv.hip), shared by tests/test_hip_depthwise.py,
tests/test_depthwise_host.py and tools/dwconv_bench.py: ``(N, C, H, W, K, stride, pad)``."""

CASES = [
    (2, 5, 7, 9, 3, 1, 1),       # odd everything, unaligned rows
    (1, 3, 8, 8, 3, 2, 1),       # stride 2 on even sizes
    (2, 4, 9, 7, 3, 2, 1),       # stride 2 on odd sizes
    (1, 2, 5, 5, 5, 1, 2),       # K = 5
    (1, 2, 7, 7, 7, 1, 3),       # K = 7
    (1, 1, 3, 3, 3, 1, 0),       # no padding, a single output pixel
    (1, 2, 4, 4, 3, 1, 0),       # no padding
    (2, 8, 1, 1, 3, 1, 1),       # 1 x 1 map: only the centre tap lies inside
    (3, 33, 16, 16, 3, 1, 1),    # aligned rows, more channels than one workgroup's share
    (1, 2, 2, 130, 3, 1, 1),     # a row longer than one strip
    (1, 1, 70, 3, 3, 2, 1),      # many short rows: strip boundaries along y
    (5, 3, 37, 41, 3, 1, 1),     # the gradient's slab boundaries
]


def out_size(h: int, w: int, k: int, stride: int, pad: int):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def case_id(case) -> str:
    return "n%d_c%d_%dx%d_k%d_s%d_p%d" % tuple(case)


class SepNet:
    """Builder of the depthwise-separable test network: dense 3 x 3 stem, dw 3 x 3, pw 1 x 1, dw 5 x 5 stride 2 with a bias, pw 1 x 1,
    pool, fc (a function, so that importing this file needs no torch)."""

    @staticmethod
    def build(classes: int = 10):
        import torch
        from torch import nn

        class _SepNet(nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = nn.Conv2d(3, 8, 3, padding=1, bias=False)
                self.bn1 = nn.BatchNorm2d(8)
                self.relu1 = nn.ReLU()
                self.dw1 = nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False)
                self.bn2 = nn.BatchNorm2d(8)
                self.relu2 = nn.ReLU()
                self.pw1 = nn.Conv2d(8, 16, 1, bias=False)
                self.bn3 = nn.BatchNorm2d(16)
                self.relu3 = nn.ReLU()
                self.dw2 = nn.Conv2d(16, 16, 5, stride=2, padding=2, groups=16, bias=True)
                self.bn4 = nn.BatchNorm2d(16)
                self.relu4 = nn.ReLU()
                self.pw2 = nn.Conv2d(16, 12, 1, bias=False)
                self.relu5 = nn.ReLU()
                self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
                self.fc = nn.Linear(12, classes)

            def forward(self, x):
                x = self.relu1(self.bn1(self.conv1(x)))
                x = self.relu2(self.bn2(self.dw1(x)))
                x = self.relu3(self.bn3(self.pw1(x)))
                x = self.relu4(self.bn4(self.dw2(x)))
                x = self.relu5(self.pw2(x))
                return self.fc(torch.flatten(self.avgpool(x), 1))

        return _SepNet()
