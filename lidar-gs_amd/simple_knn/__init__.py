"""`simple_knn` -- drop-in for the third-party CUDA extension that the reference's scene/gaussian_model.py:21 imports
(`from simple_knn._C import distCUDA2`).  With lidar-gs_amd/ on PYTHONPATH that import resolves here and runs on the HIP kernel of
include/lidargs_knn.h."""
