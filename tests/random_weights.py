"""TEST INFRASTRUCTURE: the seeded random 508-key state-dict of test_random_weights_against_oracle (He-style conv weights, BatchNorm
statistics away from the identity, negative biases), shared with the fp16 launch replay."""
import torch


def random_state_dict(seed, num_out=24, input_channel=1):
    from yolo_fastest_amd import packer
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, kind, cin, cout, k, stride, relu in packer.layer_table(num_out, input_channel):
        if kind == packer.KIND_HEAD:
            sd[name + ".weight"] = torch.randn((cout, cin, 1, 1), generator=g) * (1.0 / cin) ** 0.5
            sd[name + ".bias"] = torch.randn((cout,), generator=g) * 0.5
            continue
        shape = {packer.KIND_PW: (cout, cin, 1, 1), packer.KIND_DENSE: (cout, cin, k, k), packer.KIND_DW: (cout, 1, k, k),
                 packer.KIND_DECONV: (cin, cout, 2, 2)}[kind]
        fan = cin * (k * k if kind == packer.KIND_DENSE else 1) if kind != packer.KIND_DW else k * k
        sd[name + ".0.weight"] = torch.randn(shape, generator=g) * (1.0 / fan) ** 0.5   # keeps the 86-layer chain in range
        sd[name + ".1.weight"] = 0.5 + torch.rand((cout,), generator=g)
        sd[name + ".1.bias"] = torch.randn((cout,), generator=g) * 0.2
        sd[name + ".1.running_mean"] = torch.randn((cout,), generator=g) * 0.2
        sd[name + ".1.running_var"] = 0.5 + torch.rand((cout,), generator=g)
        sd[name + ".1.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return sd
