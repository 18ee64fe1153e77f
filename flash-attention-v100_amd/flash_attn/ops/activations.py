"""`flash_attn.ops.activations` with upstream's names and argument lists; the implementation is the `fa_act_mul` / `fa_act_mul_bwd`
HIP kernels (flash_attn_mi355.act_mul, which states the fp32 formulas and the special values).  fp16 / bf16 GPU tensors
`[..., N]`; every function is one launch.

    swiglu(x, y)          silu(x) * y, differentiable in x and y        swiglu_fwd(x, y) / swiglu_bwd(x, y, g) -> (dx, dy)
    gelu_fwd(x)           upstream's gelu here is the TANH form         gelu_bwd(g, x);   fast_gelu_impl(x): the same, differentiable
    sqrelu_fwd(x)         relu(x)^2                                     sqrelu_bwd(g, x)
    relu_bwd(g, x)        g where x > 0, else 0 - upstream passes g at x == 0 as well, this takes torch's relu'(0) = 0

The biased forms (`bias_gelu`, `bias_gelu_back`, `bias_gelu_impl`) are not defined: a bias gradient is a column sum, which the
element-wise kernel does not form."""
from flash_attn_mi355 import act_mul as _am


def swiglu_fwd(x, y):
    return _am.act_mul_forward(x, y, activation="silu")


def swiglu_bwd(x, y, g):
    return _am.act_mul_backward(g, x, y, activation="silu")


def swiglu(x, y):
    return _am.act_mul(x, y, activation="silu")


def gelu_fwd(x):
    return _am.act_mul_forward(x, activation="gelu_tanh")


def gelu_bwd(g, x):
    return _am.act_mul_backward(g, x, activation="gelu_tanh")[0]


def fast_gelu_impl(x):
    return _am.act_mul(x, activation="gelu_tanh")


def relu_bwd(g, x):
    return _am.act_mul_backward(g, x, activation="relu")[0]


def sqrelu_fwd(x):
    return _am.act_mul_forward(x, activation="relu2")


def sqrelu_bwd(g, x):
    return _am.act_mul_backward(g, x, activation="relu2")[0]
