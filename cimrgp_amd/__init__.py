"""cimrgp_amd -- MI355X-native dense covariance/posterior path of ciMRGP.

Host-side mirror of the reference's module layout (``IndexSetGenerator``,
``KernelClass``, ``Posteriors``, ``RegressionInput``, ``Inputs``, ``MRGP``)
over hand-written HIP kernels reached through the C ABI of ``libcimrgp.so``
(include/cimrgp.h).  No CPU fallback: importing the package does not need a
GPU, computing does.
"""
from .IndexSetGenerator import IndexSetUniform
from .KernelClass import RBFKernel, DenseMaternKernel, MaternKernel, LaplacianEigenpairs, SparseKernel
from .BasisInterval import BasisInterval
from .RegressionInput import RegressionMethod, GP_RBF, GP_Matern, SparseGP, SGP_FITC, SparseGP_RBF, SparseGP_RBFLinear, SVIGP_RBF, BGPLVM
from .Inputs import space_filling_order
from .Posteriors import DensePosterior, DenseBlock
from .Sparse import SparseBlock, SparsePosterior
from .SVGP import SVGPBlock
from .Psi import UncertainInputBlock
from .MRGP import MultiResolutionGaussianProcess
from . import _lib, device, dist

__all__ = ["IndexSetUniform", "RBFKernel", "DenseMaternKernel", "MaternKernel", "LaplacianEigenpairs", "BasisInterval", "RegressionMethod",
           "GP_RBF", "GP_Matern", "SparseGP", "SGP_FITC", "SparseGP_RBF", "SparseGP_RBFLinear", "SVIGP_RBF", "BGPLVM", "DensePosterior", "DenseBlock", "SparseBlock", "SVGPBlock", "UncertainInputBlock", "SparseKernel", "SparsePosterior", "MultiResolutionGaussianProcess", "space_filling_order", "device", "dist"]
