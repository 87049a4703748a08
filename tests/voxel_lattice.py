"""The smallest cloud at which pcl::VoxelGrid's key arithmetic can go wrong, for the tests of dgs_voxel_grid_filter and
dgs_cloud_assign_batch: points on the faces of the cells and one float to either side of them."""
import numpy as np


def lattice_cloud(leaf: float) -> np.ndarray:
    """[1029, 4] float32: the 343 points k * leaf (float32 product), k = -3 .. 3 on each axis, then every one of them moved one float up
    on all three axes, then one float down (np.nextafter).  min_b is negative, every cell face between -3 leaf and 3 leaf carries points,
    and a cell holds a few points.  leaf 0.5 has an exact inverse, leaf 0.1 has not."""
    k = np.arange(-3, 4, dtype=np.float32) * np.float32(leaf)
    on = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([on, np.nextafter(on, np.float32(np.inf)), np.nextafter(on, np.float32(-np.inf))])
    out = np.ones((xyz.shape[0], 4), np.float32)
    out[:, :3] = xyz
    return out
