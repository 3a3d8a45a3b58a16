"""The MicFormer Head the sliding-window tests use as a real predictor: every parameter filled from oracle/fill.py, on the GPU, in
eval mode."""
import torch


def filled_head(E, depths):
    from oracle import fill
    import micformer_amd.models.MICFormer_self as M
    head = M.Head(embed_dim=E, num_classes=8, depths=depths)
    with torch.no_grad():
        for name, t in head.state_dict().items():
            t.copy_(fill.fill_tensor(name, t))
    return head.cuda().eval()
