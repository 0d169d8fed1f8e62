import ctypes as C

import numpy as np
import torch

from suo_slam_amd import _lib


def run_backbone_from_staged(net, xin_nhwc48):
    """xin: numpy [L,256,256,48] -> numpy logits [L,41,64,64] through suo_net_backbone."""
    x = torch.from_numpy(np.ascontiguousarray(xin_nhwc48, np.float32)).cuda()
    L = x.shape[0]
    out = torch.empty((L, 41, 64, 64), device="cuda")
    _lib.check(_lib.lib().suo_net_backbone(net._h, C.c_void_p(x.data_ptr()), L, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "suo_net_backbone")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_backbone_from_device_crops(net, base, sel):
    """base: device tensor [k,256,256,48] of k distinct staged crops; sel: L indices into it -> DEVICE logits [L,41,64,64] through suo_net_backbone.  The
    [L,256,256,48] input is gathered on the device (base[sel]): at 129 crops it is 1.6 GB, which run_backbone_from_staged would push through the host."""
    assert base.is_cuda and base.dtype == torch.float32 and tuple(base.shape[1:]) == (256, 256, 48)
    x = base.index_select(0, torch.as_tensor(list(sel), dtype=torch.long, device=base.device)).contiguous()
    L = x.shape[0]
    out = torch.empty((L, 41, 64, 64), device=base.device)
    _lib.check(_lib.lib().suo_net_backbone(net._h, C.c_void_p(x.data_ptr()), L, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "suo_net_backbone")
    torch.cuda.synchronize()
    return out
