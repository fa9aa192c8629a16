"""Import-name shim package for the two pytorch3d modules the reference uses: `pytorch3d.ops` (knn_points) and
`pytorch3d.transforms` (matrix_to_quaternion, quaternion_to_matrix).  Nothing else of pytorch3d exists here."""
