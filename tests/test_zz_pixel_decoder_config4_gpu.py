"""GPU: MSDeformAttnPixelDecoder alone at the size of BASELINE configs[4] (Mask2Former on ViT-Adapter-L, 800 x 1344, one
image per GPU): random feats in place of a backbone run, four 1024-channel maps at strides 4 .. 32, forward + backward
under bf16 autocast; then the same step captured into a HIP graph and replayed once."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = ((200, 336), (100, 168), (50, 84), (25, 42))


def test_configs4_pixel_decoder_bf16_eager_and_graph():
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(0)
    m = MSDeformAttnPixelDecoder(in_channels=(1024,) * 4)
    m.init_weights()                            # on the host, then moved: the attention's init makes new parameters
    m = m.cuda().train()
    with torch.no_grad():                       # away from the all-zero initial offsets / weights
        for layer in m.encoder.layers:
            layer.attentions[0].sampling_offsets.weight.normal_(0, 0.02)
            layer.attentions[0].attention_weights.weight.normal_(0, 0.05)
    g = torch.Generator(device='cuda').manual_seed(4)
    feats = [torch.randn(1, 1024, h, w, device='cuda', generator=g).to(torch.bfloat16).requires_grad_(True) for h, w in SIZES]

    def step():
        m.zero_grad(set_to_none=True)
        for f in feats:
            f.grad = None
        with torch.autocast('cuda', dtype=torch.bfloat16):
            mask_feature, ms = m(feats)
        loss = mask_feature.float().pow(2).mean() + sum(o.float().pow(2).mean() for o in ms)
        loss.backward()
        return loss.detach(), mask_feature, ms

    # every step, the first included, runs on a side stream, as bench.py's do: the AccumulateGrad nodes of the parameters
    # and of the feats are made by the first backward and belong to the stream it ran on - on the default (null) stream they
    # would pull that stream into the capture below, which a capture cannot hold
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss, mask_feature, ms = step()
        assert tuple(mask_feature.shape) == (1, 256, 200, 336)
        assert [tuple(o.shape) for o in ms] == [(1, 256, 25, 42), (1, 256, 50, 84), (1, 256, 100, 168)]
        assert bool(torch.isfinite(loss))
        for mod in (m.lateral_convs, m.output_convs, m.mask_feature, m.level_encoding, m.input_convs, m.encoder):
            grads = [p.grad for p in mod.parameters()]
            assert grads and all(gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0 for gr in grads)
        for f in feats:
            assert f.grad is not None and bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0
        eager = float(loss)
        del loss, mask_feature, ms
        step()                                  # once more: every library algorithm is chosen
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    # the same step captured and replayed once: nothing in it reads back to the host.  Nothing made before the capture is
    # released inside it: the gradients are cleared first.
    m.zero_grad(set_to_none=True)
    for f in feats:
        f.grad = None
    # the parameters' AccumulateGrad nodes were made on the side stream; the capture stream differs by design.  The warning
    # is a process-wide setting (on by default): switched off for the capture alone.
    quiet = getattr(torch.autograd.graph, 'set_warn_on_accumulate_grad_stream_mismatch', None)
    if quiet is not None:
        quiet(False)
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            graph_loss = step()[0]
        graph.replay()
        torch.cuda.synchronize()
    finally:
        if quiet is not None:
            quiet(True)
    assert float(graph_loss) == eager, (float(graph_loss), eager)
