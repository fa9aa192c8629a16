"""Import-name shim: `from pytorch3d.transforms import matrix_to_quaternion, quaternion_to_matrix` [REF utils/camera_utils.py:17,
272-275].  Small torch functions on any device, CPU included (the reference calls them on `torch.from_numpy` output).
Quaternions are real-part first (w, x, y, z).  matrix_to_quaternion returns the representative with w >= 0.  Parity with the
real pytorch3d is unpinned: the package is absent, so this follows its documented contract and has never been compared
against it."""
import torch


def quaternion_to_matrix(quaternions):
    """[..., 4] (w, x, y, z), any norm (normalised here) -> [..., 3, 3] rotation matrices."""
    w, x, y, z = torch.unbind(quaternions, -1)
    s = 2.0 / (quaternions * quaternions).sum(-1)
    m = torch.stack((1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w),
                     s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w),
                     s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)), -1)
    return m.reshape(quaternions.shape[:-1] + (3, 3))


def matrix_to_quaternion(matrix):
    """[..., 3, 3] rotation matrices -> [..., 4] unit quaternions (w, x, y, z), w >= 0.  Each matrix uses the best conditioned of
    the four closed forms (the one whose diagonal term is largest)."""
    if matrix.shape[-2:] != (3, 3):
        raise ValueError(f"matrix_to_quaternion: [..., 3, 3] expected, got {tuple(matrix.shape)}")
    m = matrix
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    # 4 w^2, 4 x^2, 4 y^2, 4 z^2
    t = torch.stack((1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22), -1)
    r = torch.sqrt(t.clamp_min(0.0))
    d21, d02, d10 = m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]
    s21, s02, s10 = m[..., 2, 1] + m[..., 1, 2], m[..., 0, 2] + m[..., 2, 0], m[..., 1, 0] + m[..., 0, 1]
    # candidate k: component k is r_k / 2, the others follow from the off-diagonal sums / differences divided by 2 r_k
    cand = torch.stack((torch.stack((t[..., 0], d21, d02, d10), -1),
                        torch.stack((d21, t[..., 1], s10, s02), -1),
                        torch.stack((d02, s10, t[..., 2], s21), -1),
                        torch.stack((d10, s02, s21, t[..., 3]), -1)), -2)
    cand = cand / (2.0 * r.clamp_min(1e-12))[..., None]
    best = torch.argmax(t, -1)
    q = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    q = q / torch.linalg.vector_norm(q, dim=-1, keepdim=True)
    return torch.where(q[..., :1] < 0, -q, q)
