"""torchvision's RandomPerspective parameter draws and its coefficient solve, restated on torch's own generator and lstsq
(torchvision is not installed): what `transformations_code.apply_perspective_warp` (the tensor path, `ops.perspective`) and
`transform_list.perspective_list` (the PIL path) share.  Host only."""
from __future__ import annotations

import torch


def _perspective_endpoints(width: int, height: int, distortion_scale: float):
    """RandomPerspective.get_params: eight torch.randint draws from torch's global CPU generator,
    in torchvision's order (top-left x, y; top-right; bottom-right; bottom-left)."""
    def randint(lo, hi):
        return int(torch.randint(lo, hi, size=(1,)).item())
    half_height, half_width = height // 2, width // 2
    dw, dh = int(distortion_scale * half_width), int(distortion_scale * half_height)
    topleft = [randint(0, dw + 1), randint(0, dh + 1)]
    topright = [randint(width - dw - 1, width), randint(0, dh + 1)]
    botright = [randint(width - dw - 1, width), randint(height - dh - 1, height)]
    botleft = [randint(0, dw + 1), randint(height - dh - 1, height)]
    startpoints = [[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]]
    return startpoints, [topleft, topright, botright, botleft]


def _perspective_coeffs(startpoints, endpoints):
    """torchvision F._get_perspective_coeffs: fp64 least squares (gels), cast to fp32."""
    a = torch.zeros(2 * len(startpoints), 8, dtype=torch.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]], dtype=torch.float64)
        a[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]], dtype=torch.float64)
    b = torch.tensor(startpoints, dtype=torch.float64).view(8)
    return torch.linalg.lstsq(a, b, driver="gels").solution.to(torch.float32).tolist()
