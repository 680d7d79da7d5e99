"""The reference's src/tools on the HIP path: mesh culling (cull_mesh) and the 3D reconstruction metrics (eval_recon)."""
