"""Import-name shim package for the reference's `simple_knn` CUDA extension (see `simple_knn._C`)."""
