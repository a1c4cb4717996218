"""Plain-torch restatement of FaceNet's InceptionResnetV1 in eval mode (F.conv2d, F.batch_norm, F.max_pool2d ...), over a flat state
dict with facenet_pytorch's key names, in whatever dtype the state dict and the input have (fp64 = the reference for the HIP
embedder, fp32 = the yardstick of the ordinary fp32 error).  Written from the network's published structure, not from the engine:
nothing here is folded, merged or repacked.  Also the hand-written manifest's generator (`manifest()`) and a seeded weight generator
that keeps activations O(1)."""
import torch
import torch.nn.functional as F

EPS = 1e-3


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


# (name, in, out, kernel, stride, padding) of every BasicConv2d, and (name, in, out) of every plain 1 x 1 convolution
def _block35(p):
    return ([(p + "branch0", 256, 32, 1, 1, 0),
             (p + "branch1.0", 256, 32, 1, 1, 0), (p + "branch1.1", 32, 32, 3, 1, 1),
             (p + "branch2.0", 256, 32, 1, 1, 0), (p + "branch2.1", 32, 32, 3, 1, 1), (p + "branch2.2", 32, 32, 3, 1, 1)],
            (p + "conv2d", 96, 256))


def _block17(p):
    return ([(p + "branch0", 896, 128, 1, 1, 0),
             (p + "branch1.0", 896, 128, 1, 1, 0), (p + "branch1.1", 128, 128, (1, 7), 1, (0, 3)),
             (p + "branch1.2", 128, 128, (7, 1), 1, (3, 0))],
            (p + "conv2d", 256, 896))


def _block8(p):
    return ([(p + "branch0", 1792, 192, 1, 1, 0),
             (p + "branch1.0", 1792, 192, 1, 1, 0), (p + "branch1.1", 192, 192, (1, 3), 1, (0, 1)),
             (p + "branch1.2", 192, 192, (3, 1), 1, (1, 0))],
            (p + "conv2d", 384, 1792))


STEM = [("conv2d_1a", 3, 32, 3, 2, 0), ("conv2d_2a", 32, 32, 3, 1, 0), ("conv2d_2b", 32, 64, 3, 1, 1), ("conv2d_3b", 64, 80, 1, 1, 0),
        ("conv2d_4a", 80, 192, 3, 1, 0), ("conv2d_4b", 192, 256, 3, 2, 0)]
MIXED_6A = [("mixed_6a.branch0", 256, 384, 3, 2, 0), ("mixed_6a.branch1.0", 256, 192, 1, 1, 0), ("mixed_6a.branch1.1", 192, 192, 3, 1, 1),
            ("mixed_6a.branch1.2", 192, 256, 3, 2, 0)]
MIXED_7A = [("mixed_7a.branch0.0", 896, 256, 1, 1, 0), ("mixed_7a.branch0.1", 256, 384, 3, 2, 0),
            ("mixed_7a.branch1.0", 896, 256, 1, 1, 0), ("mixed_7a.branch1.1", 256, 256, 3, 2, 0),
            ("mixed_7a.branch2.0", 896, 256, 1, 1, 0), ("mixed_7a.branch2.1", 256, 256, 3, 1, 1), ("mixed_7a.branch2.2", 256, 256, 3, 2, 0)]


def layers():
    """(basic, plain): every BasicConv2d and every plain convolution of the network, in module order."""
    basic, plain = list(STEM), []
    for i in range(5):
        b, p = _block35(f"repeat_1.{i}.")
        basic += b
        plain.append(p)
    basic += MIXED_6A
    for i in range(10):
        b, p = _block17(f"repeat_2.{i}.")
        basic += b
        plain.append(p)
    basic += MIXED_7A
    for pre in [f"repeat_3.{i}." for i in range(5)] + ["block8."]:
        b, p = _block8(pre)
        basic += b
        plain.append(p)
    return basic, plain


def manifest(num_classes=None):
    """key -> shape (list) of the state dict."""
    m = {}
    basic, plain = layers()
    for name, ci, co, k, _, _ in basic:
        kh, kw = _pair(k)
        m[name + ".conv.weight"] = [co, ci, kh, kw]
        for s in ("weight", "bias", "running_mean", "running_var"):
            m[name + ".bn." + s] = [co]
        m[name + ".bn.num_batches_tracked"] = []
    for name, ci, co in plain:
        m[name + ".weight"] = [co, ci, 1, 1]
        m[name + ".bias"] = [co]
    m["last_linear.weight"] = [512, 1792]
    for s in ("weight", "bias", "running_mean", "running_var"):
        m["last_bn." + s] = [512]
    m["last_bn.num_batches_tracked"] = []
    if num_classes is not None:
        m["logits.weight"] = [num_classes, 512]
        m["logits.bias"] = [num_classes]
    return m


def seeded_state(seed, dtype=torch.float32):
    """He-scaled convolution weights, gamma in U[0.5, 1.5], beta and running mean ~ N(0, 0.1), running var in U[0.5, 1.5]."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in manifest().items():
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.zeros((), dtype=torch.int64)
        elif key.endswith("running_var") or (".bn." in key or key.startswith("last_bn.")) and key.endswith(".weight"):
            sd[key] = (0.5 + torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype)
        elif key.endswith("running_mean") or key.endswith(".bias"):
            sd[key] = (0.1 * torch.randn(shape, generator=g, dtype=torch.float64)).to(dtype)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[key] = (torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).to(dtype)
    return sd


def to_dtype(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def basic(sd, name, x, stride=1, padding=0):
    x = F.conv2d(x, sd[name + ".conv.weight"], None, _pair(stride), _pair(padding))
    x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                     False, 0.1, EPS)
    return F.relu(x)


def _seq(sd, specs, x):
    for name, _, _, _, s, p in specs:
        x = basic(sd, name, x, s, p)
    return x


def _res_block(sd, spec, x, scale, relu=True):
    bas, (pname, _, _) = spec
    branches, cur = [], None
    for item in bas:                       # group by branch index
        br = item[0].split("branch")[1][0]
        if br != cur:
            branches.append([])
            cur = br
        branches[-1].append(item)
    out = torch.cat([_seq(sd, b, x) for b in branches], 1)
    out = F.conv2d(out, sd[pname + ".weight"], sd[pname + ".bias"])
    out = out * scale + x
    return F.relu(out) if relu else out


def stage_sizes(n):
    """Side lengths along one axis after conv2d_1a, 2a, 2b, maxpool_3a, 3b, 4a, 4b, mixed_6a, mixed_7a; raises when one is < 1."""
    out = []
    for k, s, p in ((3, 2, 0), (3, 1, 0), (3, 1, 1), (3, 2, 0), (1, 1, 0), (3, 1, 0), (3, 2, 0), (3, 2, 0), (3, 2, 0)):
        if n + 2 * p < k:
            raise ValueError("input too small")
        n = (n + 2 * p - k) // s + 1
        out.append(n)
    return out


def forward(sd, x):
    """x [T, 3, H, W], standardised -> [T, 512] unit rows."""
    x = _seq(sd, STEM[:3], x)
    x = F.max_pool2d(x, 3, 2)
    x = _seq(sd, STEM[3:], x)
    for i in range(5):
        x = _res_block(sd, _block35(f"repeat_1.{i}."), x, 0.17)
    x = torch.cat([basic(sd, "mixed_6a.branch0", x, 2, 0), _seq(sd, MIXED_6A[1:], x), F.max_pool2d(x, 3, 2)], 1)
    for i in range(10):
        x = _res_block(sd, _block17(f"repeat_2.{i}."), x, 0.10)
    x = torch.cat([_seq(sd, MIXED_7A[0:2], x), _seq(sd, MIXED_7A[2:4], x), _seq(sd, MIXED_7A[4:7], x), F.max_pool2d(x, 3, 2)], 1)
    for i in range(5):
        x = _res_block(sd, _block8(f"repeat_3.{i}."), x, 0.20)
    x = _res_block(sd, _block8("block8."), x, 1.0, relu=False)
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    x = F.linear(x, sd["last_linear.weight"])
    x = F.batch_norm(x, sd["last_bn.running_mean"], sd["last_bn.running_var"], sd["last_bn.weight"], sd["last_bn.bias"], False, 0.1, EPS)
    return F.normalize(x, p=2.0, dim=1)


def standardize(u):
    return (u - 127.5) / 128.0
